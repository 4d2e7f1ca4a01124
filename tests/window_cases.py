"""Loci that sit on the caps of a tile's descriptor, and the model that says where they sit.  No GPU, no tests: tests/test_window_cases_cpu.py
proves every case here before tests/test_gpu_window_limits.py runs it.

A tile's descriptor (make_descriptor in l2r_window.hip.h, its twin in k_pass_a) is three things: the WINDOW (the transcripts from the
tile's cursor up to the first one that lies behind the tile's span, less those entirely in front of it), the SLICES of the START / END
site dictionaries over the tile's 512-base buckets, and the bucket count itself.  The model below restates them from the transcripts and
the reads; the dictionary part is the one tests/test_gpu_chunk_limits.py has used since its cases were written (it imports it from here).

    window        WIN_TX = 32 members on 32-bit masks, WIDE_MEMBERS = 63 on 64-bit masks           cases "win_*"
    slices        SLAB_KEY_CAP = 168 START / END entries (slab, tile), KEY_CAP = 224 (classic)       cases "st_*" / "en_*"
    buckets       DIR_CAP = 384                                                                      cases "span_*"
    window scan   WIN_SCAN_TRIPS * 64 = 4096 transcripts behind the cursor                          cases "scan_*"
    -d            DIS_MASK_MAX = 64                                                                  cases "dis_*"
    positions     TILE_POS_CAP = 2400 (k_tile), SLAB_POS_CAP = 2536 (k_probe_slab) exons of a tile   cases "pos_*"
    rows          SLAB_ROWS = 24 exons of a read; 255 exons: the tile is never exact                 cases "rows_*"

Construction shared by the window, slice, scan and -d cases: every read begins in bucket LO_B and ends in bucket HI_B, every multi-exon
transcript of the locus has its exon F in LO_B and its last exon in HI_B, so every tile has the same buckets, the same window and the
same slices however the reads are cut into tiles.  In front of F every isoform has an exon P in bucket LO_B - 1: a read is only "known"
when its first base is an annotated acceptor (Q1, src/update_gtf.c:746), so the known reads begin at F's first base.  The locus is
14 kb long: a single-exon read over it stays below the 2^14 bases a slab row holds."""
import bisect
from collections import defaultdict, namedtuple

import numpy as np

from tests import upload_plan_restatement as plan
from tests.test_gpu_edges import _chain          # (exons -> position and CIGAR; importing the module needs no GPU)

SITE_SHIFT = 9
WIN_TX, WIDE_MEMBERS, SLAB_KEY_CAP, KEY_CAP, DIR_CAP, WIN_SCAN, DIS_MASK_MAX = 32, 63, 168, 224, 384, 4096, 64
TILE_POS_CAP, SLAB_POS_CAP, SLAB_ROWS, NEVER_EXACT = 2400, 2536, 24, 255
LO_B, HI_B = 200, 228
B0, B1 = LO_B << SITE_SHIFT, HI_B << SITE_SHIFT
M, N_ = 0, 3


# ---- the model: build_dict (l2r_tables.hip.h), the window scan and the slice bounds of make_descriptor (l2r_window.hip.h)

def _parts(pairs, singles):
    """Entries of one dictionary as sorted keys (tid, k1, k2), one per part.  A key's members are its pairs and the singles with the
    same (tid, k1); a part starts at the lowest member left and takes every member less than 64 past it."""
    members, by_k1 = defaultdict(list), defaultdict(list)
    for tid, k1, k2, tx in pairs:
        members[(tid, k1, k2)].append(tx)
    for tid, k1, tx in singles:
        by_k1[(tid, k1)].append(tx)
    ent = []
    for key in sorted(members):
        p, s = sorted(members[key]), sorted(by_k1[key[:2]])
        while p or s:
            lo = min(p[:1] + s[:1])
            p, s = [t for t in p if t - lo >= 64], [t for t in s if t - lo >= 64]
            ent.append(key)
    return ent


def _dictionaries(txs):
    """START (exons + acceptors) and END (junctions + donors) entries; transcripts of one exon or without a chromosome enter none."""
    kx, ka, kj, kd = [], [], [], []
    for i, (tid, _rev, ex) in enumerate(txs):
        if tid < 0 or len(ex) < 2:
            continue
        for k, (s, e) in enumerate(ex):
            kx.append((tid, s, e, i))
            if k + 1 < len(ex):
                kd.append((tid, e, i))
                kj.append((tid, e, ex[k + 1][0], i))
            if k:
                ka.append((tid, s, i))
    nb = defaultdict(int)                       # buckets per chromosome: up to its largest key 1, and exon end
    for tid, k1, k2, _ in kx:
        nb[tid] = max(nb[tid], (max(k1, k2) >> SITE_SHIFT) + 1)
    for tid, k1, _k2, _ in kj:
        nb[tid] = max(nb[tid], (k1 >> SITE_SHIFT) + 1)
    return _parts(kx, ka), _parts(kj, kd), nb


def ref_len(ops):
    return sum(l for l, op in ops if op in plan.REF_OPS)


def tiles_of(rows, slab=True, min_intron=3, max_delet=50):
    """[(first read, one past the last)] of the upload's tiles (tests/upload_plan_restatement.py), and the plan."""
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r[3]) for r in rows], out=off[1:])
    cig = [(l << 4) | op for r in rows for l, op in r[3]]
    p = plan.upload_plan([r[0] for r in rows], [r[1] for r in rows], off, cig, min_intron=min_intron, max_delet=max_delet, want_slab=slab)
    f = p["tile_first"]
    return [(f[t], f[t + 1]) for t in range(p["n_tiles"])], p


def window(txs, tid, tlo, thi):
    """(cursor, members, transcripts the scan looks at up to and with the one that stops it -- None: the annotation ends first).
    The cursor is the first transcript whose running maximum of (tid, end) lies behind (tid, tlo); the scan stops at the first
    transcript comp_trans places behind the span (a larger tid, or a start at or behind thi); a transcript with a smaller tid (-1:
    none) or one that ends at or before tlo is skipped."""
    cur, run = len(txs), None
    for i, (t, _rev, ex) in enumerate(txs):
        key = (t, ex[-1][1])
        run = key if run is None or key > run else run
        if run > (tid, tlo):
            cur = i
            break
    members = []
    for i in range(cur, len(txs)):
        t, _rev, ex = txs[i]
        s, e = ex[0][0], ex[-1][1]
        if tid < t or (tid == t and thi <= s):
            return cur, members, i - cur + 1
        if t < tid or (e <= tlo and s < tlo):
            continue
        members.append(i)
    return cur, members, None


class Dictionaries:
    def __init__(self, txs):
        self.st, self.en, self.nb = _dictionaries(txs)
        self._stb = [(t, k1 >> SITE_SHIFT) for t, k1, _ in self.st]
        self._enb = [(t, k1 >> SITE_SHIFT) for t, k1, _ in self.en]

    def slices(self, tid, tlo, thi, dis=0):
        """(nbk, START entries, END entries) of a tile's descriptor: START from the reach-back directory of lo (the first entry whose
        exon reaches into bucket lo from an earlier one), END from the plain directory; -d widens the span on both sides."""
        n = self.nb[tid]
        lo, hi = min(max(tlo - dis, 0) >> SITE_SHIFT, n - 1), min(max(thi + dis, 0) >> SITE_SHIFT, n - 1)
        s0, s1 = bisect.bisect_left(self._stb, (tid, lo)), bisect.bisect_left(self._stb, (tid, hi + 1))
        for i, (t, k1, k2) in enumerate(self.st[:s0]):
            if t == tid and (k1 >> SITE_SHIFT) < lo <= min(k2 >> SITE_SHIFT, n - 1) and (i == 0 or self.st[i - 1] != self.st[i]):
                s0 = i
                break
        e0, e1 = bisect.bisect_left(self._enb, (tid, lo)), bisect.bisect_left(self._enb, (tid, hi + 1))
        return hi - lo + 1, self.st[s0:s1], self.en[e0:e1]


Tile = namedtuple("Tile", "first last tlo thi cursor members scanned nbk st en")


def describe(txs, rows, dis=0, slab=True, **thresholds):
    """The descriptor of every tile of `rows` (sorted (tid, pos0, rev, ops))."""
    dic = Dictionaries(txs)
    out = []
    for a, b in tiles_of(rows, slab, **thresholds)[0]:
        tid, tlo = rows[a][0], rows[a][1] + 1
        thi = max(r[1] + ref_len(r[3]) for r in rows[a:b])
        cur, members, scanned = window(txs, tid, tlo, thi)
        nbk, st, en = dic.slices(tid, tlo, thi, dis)
        out.append(Tile(a, b, tlo, thi, cur, members, scanned, nbk, st, en))
    return out


# ---- exons of the loci

def P(g):
    return (B0 - 300, B0 - 250 + g)


def F(g):
    return (B0 + 150 + 2 * g, B0 + 300 + 4 * g)                  # g < 48


def L(g):
    return (B1 + 20 + 4 * g, B1 + 240 + 4 * g)                   # g < 64


def inner(k):
    return (103_000 + 52 * k, 103_029 + 52 * k)                  # k < 263: inside buckets LO_B + 1 .. HI_B - 1


STOP = (0, 0, [(150_000, 150_100), (150_300, 150_400)])         # the transcript behind the span that ends every window scan
EARLY = B0 + 10                                                  # first base of the reads that begin in front of every F


def _finish(rows):
    """(pos0, ops) in the order made -> (tid, pos0, rev, ops) sorted, strands alternating; and where each row went."""
    order = sorted(range(len(rows)), key=lambda i: rows[i][0])
    at = {orig: new for new, orig in enumerate(order)}
    return [(0, rows[i][0], i & 1, rows[i][1]) for i in order], at


Case = namedtuple("Case", "name family txs rows params levels meta")


def _spec(case_name, build, *args, **kw):
    """(name, the call that builds the case): the tests are parametrised by name, and a case is built when a test asks for it"""
    return case_name, (lambda: build(*args, **kw))


def _locus_rows(isos, n, seed, edge, late=0, single_end=None, phantom_donors=()):
    """Reads over the isoforms `isos` (exon lists without P): of every eight one each of
        0  an isoform from F's first base (an acceptor: known), its last exon shortened
        1  ... isoform 0, the window's member 0          2  ... `edge`, the chain of the window's last member
        3  every site moved by 4 bases (no known site)   4  one donor moved (known sites, not known)
        5  a skipped exon                                6  a single exon over the locus
        7  an isoform with both outer ends moved inwards
    late > 0 (the cursor cases): the first n - late reads are kinds 3 .. 7 and begin at EARLY, in front of every F and inside the short
    transcripts at the left end of the bucket; the last `late` reads are kinds 0 .. 2, 4 and begin at or behind F's first base: behind
    every short transcript.  Returns rows and {kind: [row numbers as made]}."""
    rng = np.random.default_rng(seed)
    rows, kinds = [], defaultdict(list)
    for i in range(n):
        if late:
            kind = (0, 1, 2, 4)[i % 4] if i >= n - late else 3 + i % 5
        else:
            kind = i % 8
        iso = isos[0] if kind == 1 else edge if kind == 2 else isos[int(rng.integers(len(isos)))]
        ex = [list(x) for x in iso]
        if kind == 6:
            e = single_end[(i // 8) % len(single_end)] if single_end else B1 + 60 + int(rng.integers(0, 300))
            ex = [[ex[0][0], e]]
        else:
            ex[-1][1] -= int(rng.integers(0, 40))
        if kind == 3:
            ex[0][1] += 4
            for q in ex[1:-1]:
                q[0] += 4; q[1] += 4
            ex[-1][0] += 4
        elif kind == 4:
            ex[1 if len(ex) > 2 else 0][1] -= 5
        elif kind == 5 and len(ex) > 3:
            del ex[1 + int(rng.integers(len(ex) - 2))]
        if late and i < n - late:
            ex[0][0] = EARLY
            if phantom_donors and kind == 4:
                ex[0][1] = phantom_donors[i % len(phantom_donors)]       # (the donor of a short two-exon transcript: a known site)
        elif kind in (3, 5, 6):
            ex[0][0] = EARLY + int(rng.integers(0, 40))
        elif kind == 7:
            ex[0][0] += 1 + int(rng.integers(0, 40))
        kinds[kind].append(i)
        rows.append(_chain([tuple(x) for x in ex]))
    return rows, kinds


# ---- case 1: the window's size

GAP = (-1, 0, [(B0 + 10, B1 + 300)])                            # a transcript without a chromosome: scanned, never a member


def _isoform(i):
    """Isoform i of the window loci: groups of eight share P, F, an exon A in front and an exon C behind; every isoform has an exon X of
    its own between them -- its two junctions are nobody else's, so a read with its chain is known through it alone."""
    g, k = i // 8, i % 4
    return [F(g)] + ([inner(g)] if k & 1 else []) + [inner(10 + i)] + ([inner(80 + g)] if k & 2 else []) + [L(g)]


def _with_p(i, ex):
    """Isoform (family) i as a transcript: with the exon P in front of F, but for one in eight -- those begin with F, so the reads over
    them have the full-length evidence of a first exon that overlaps a transcript's first exon (and none is known through them)."""
    return list(ex) if i % 8 == 4 else [P(i // 8)] + list(ex)


def _window_name(n, gapped=False, edge="plain", dis=0):
    return "win_%d_%s%s%s" % (n, "gapped" if gapped else "contig", "" if edge == "plain" else "_" + edge, "_d%d" % dis if dis else "")


def window_case(n, gapped=False, edge="plain", shorts=0, dis=0, levels=(1, 3, 5), n_reads=840, name=None, twin_gap=None):
    """A locus whose window has n members: `shorts` short transcripts at the left end of LO_B, then isoforms; edge = what the last
    member is: "plain" an isoform, "single" a single-exon transcript in HI_B with single-exon reads ending over it on both sides of
    single_exon_ovlp_frac, "loose" an isoform whose exons are not in order (no TX_COMPACT), "twin" (-d > 0) an isoform with a micro-exon
    behind its own exon X: a second donor twin_gap (2 * dis: the most that one read donor can be within the tolerance of both) bases
    behind X's.  Half of the reads with its chain skip the micro-exon and end X one to twin_gap - 1 bases behind X's donor: those in
    the middle make two (annotation site, read site) pairs with the member, which the masks cannot count."""
    n_iso = n - shorts - (1 if edge == "single" else 0)
    isos = [_isoform(i) for i in range(max(n_iso, 2))]
    txs = []
    for q in range(shorts):
        txs.append((0, q & 1, [(B0 + 11 + q, B0 + 30 + q)] if q % 2 == 0 else [(B0 + 11 + q, B0 + 15 + q), (B0 + 22 + q, B0 + 30 + q)]))
    edge_chain = isos[n_iso - 1] if n_iso else isos[-1]
    for i in range(n_iso):
        ex = _with_p(i, isos[i])
        if edge == "loose" and i == n_iso - 1:
            ex = [P(i // 8), F(i // 8), inner(76), inner(75), L(i // 8)]
            edge_chain = [F(i // 8), inner(75), inner(76), L(i // 8)]
        if edge == "twin" and i == n_iso - 1:
            x = 1 + (i % 4 & 1)                                      # X in the chain: the exon of its own
            twin = (isos[i][x][1], isos[i][x][1] + (2 * dis if twin_gap is None else twin_gap))
            ex.insert(len(ex) - len(isos[i]) + x + 1, (twin[0] + 2, twin[1]))
        txs.append((0, i & 1, ex))
        if gapped and i % 3 == 2 and i + 1 < n_iso:
            txs.append(GAP)
    single_end = None
    if edge == "single":
        txs.append((0, 1, [(B1 + 100, B1 + 199)]))
        single_end = [B1 + 100 + k for k in range(70, 91)]       # 71 .. 91 of its 100 bases: around 0.8
    txs.append(STOP)
    late = 60 if shorts else 0
    donors = [B0 + 15 + q for q in range(1, shorts, 2)]
    rows, kinds = _locus_rows(isos[:max(n_iso, 2)], n_reads, 1000 * n + shorts, edge_chain, late=late, single_end=single_end, phantom_donors=donors)
    between = []
    if edge == "twin":                                           # every other read with the edge's chain: X's donor between the twins
        for q, i in enumerate(kinds[2][1::2]):
            ex = list(edge_chain)
            ex[x] = (ex[x][0], twin[0] + 1 + q % (2 * dis - 1))
            ex[-1] = (ex[-1][0], ex[-1][1] - q % 40)
            rows[i] = _chain(ex)
            between.append(i)
    rows, at = _finish(rows)
    name = name or _window_name(n, gapped, edge, dis)
    meta = dict(n_win=n, edge=edge, shorts=shorts, gapped=gapped, n_iso=n_iso, kinds={k: [at[i] for i in v] for k, v in kinds.items()})
    if edge == "twin":
        meta.update(twin=twin, between=sorted(at[i] for i in between))
    return Case(name, "window", txs, rows, dict(ss_dis=dis), levels, meta)


def window_cases():
    out = []
    for n in (31, 32, 33, 62, 63, 64):
        for kw in (dict(), dict(gapped=True), dict(edge="single"), dict(edge="loose")):
            out.append(_spec(_window_name(n, **kw), window_case, n, **kw))
    for n in (32, 63):
        for kw in (dict(dis=2), dict(gapped=True, dis=2), dict(edge="twin", dis=2)):
            out.append(_spec(_window_name(n, **kw), window_case, n, **kw))
        for k in (n - 1, n):                                     # the late reads' cursor: the last member / behind the window
            name = "win_%d_cursor_%d" % (n, k)
            out.append(_spec(name, window_case, n, shorts=k, name=name))
    return out


# ---- case 2: the dictionary slices

def _extra_chain(p, used, want):
    """Exon numbers 0 (F) .. p + 1 (L) of a transcript that adds exactly `want` junctions to `used`, which holds every (k, k + 1)."""
    chain, cur, new = [0], 0, 0
    while cur < p + 1:
        nxt = next((k for k in range(cur + 2, p + 2) if (cur, k) not in used), None) if new < want else None
        if nxt is None:
            nxt = cur + 1
        else:
            used.add((cur, nxt)); new += 1
        chain.append(nxt); cur = nxt
    return chain, new


def slice_case(which, target, members, cap, levels=(1, 3, 5)):
    """`members` transcripts, every exon and every junction in one key of one part: `which` = "st": families of one isoform P, F, inner
    exons, L, all their own -- START = 2 + inner exons per family, END = START - families.  "en": fewer families and, up to `members`,
    transcripts that jump over exons of their family: junctions nobody has, no new exon."""
    if which == "st":
        n_base, st_target = members, target
    else:
        n_base = {(32, SLAB_KEY_CAP): 16, (40, SLAB_KEY_CAP): 16, (32, KEY_CAP): 20, (40, KEY_CAP): 20}[(members, cap)]
        per = {(32, SLAB_KEY_CAP): 7, (40, SLAB_KEY_CAP): 6, (32, KEY_CAP): 8, (40, KEY_CAP): 8}[(members, cap)]
        st_target = n_base * (2 + per)
    n_inner = st_target - 2 * n_base
    ps = [n_inner // n_base + (1 if f < n_inner % n_base else 0) for f in range(n_base)]
    fams, k = [], 0
    for f, p in enumerate(ps):
        fams.append([F(f)] + [inner(k + j) for j in range(p)] + [L(f)])
        k += p
    chains = [(f, list(range(len(fams[f])))) for f in range(n_base)]
    if which == "en":
        used = [{(j, j + 1) for j in range(len(fams[f]) - 1)} for f in range(n_base)]
        rest = target - sum(len(u) for u in used)
        assert rest >= 0, rest
        for x in range(members - n_base):
            f = x % n_base
            chain, new = _extra_chain(ps[f], used[f], min(rest, 4))
            rest -= new
            chains.append((f, chain))
        assert rest == 0, rest
    txs = [(0, t & 1, ([] if f % 8 == 4 else [P(f)]) + [fams[f][j] for j in chain]) for t, (f, chain) in enumerate(chains)] + [STOP]
    assert len(txs) < 64
    isos = [[fams[f][j] for j in chain] for f, chain in chains]
    rng = np.random.default_rng(target + members)
    rows, kinds = _locus_rows(isos, 800, target * 100 + members, isos[n_base - 1])
    for i in kinds[1] + kinds[2]:                                # verbatim: the first and the last exon are entries of the START slice
        ex = isos[0] if i in kinds[1] else isos[n_base - 1]
        if rng.integers(2):
            rows[i] = _chain(ex)
    rows, at = _finish(rows)
    meta = dict(which=which, target=target, members=members, cap=cap, first_tx=0, last_tx=n_base - 1,
                first_keys=((0,) + fams[0][0], (0, fams[0][0][1], fams[0][1][0])),
                last_keys=((0,) + fams[-1][-1], (0, fams[-1][-2][1], fams[-1][-1][0])),
                kinds={k: [at[i] for i in v] for k, v in kinds.items()})
    return Case("%s_%d_m%d" % (which, target, members), "slice", txs, rows, dict(ss_dis=0), levels, meta)


def slice_cases():
    out = []
    for cap in (SLAB_KEY_CAP, KEY_CAP):
        for which in ("st", "en"):
            for target in (cap - 1, cap, cap + 1):
                for members in (24 if which == "st" else 32, 40):
                    out.append(_spec("%s_%d_m%d" % (which, target, members), slice_case, which, target, members, cap))
    return out


# ---- case 3: the bucket span

def _span_name(nbk, first_base=False, last_base=False, dis=0):
    return "span_%d%s%s%s" % (nbk, "_first_base" if first_base else "", "_last_base" if last_base else "", "_d%d" % dis if dis else "")


def span_case(nbk, first_base=False, last_base=False, dis=0):
    """Reads over six short isoforms in buckets LO_B .. LO_B + 3; one read in sixteen copies one of six transcripts whose last exon lies nbk - 1 buckets
    behind LO_B, behind one long intron: its tile's span is nbk buckets, and that exon is found through the last directory word.
    first_base: the first read begins on the first base of LO_B; last_base: the far exon ends on the last base of its bucket -- either way
    -d 1 makes the span one bucket wider."""
    far_b = LO_B + nbk - 1
    far = (far_b * 512 + 100, far_b * 512 + (511 if last_base else 300))
    near = lambda g: (B0 + 1_700 + 10 * g, B0 + 1_900 + 10 * g)
    isos = [[F(g), inner(2 * g), inner(2 * g + 1), near(g)] for g in range(6)] + [[F(g), inner(20 + g), far] for g in range(6)]
    txs = [(0, g & 1, [P(g % 6)] + ex) for g, ex in enumerate(isos)]
    txs.append((0, 0, [((LO_B + 400) * 512, (LO_B + 400) * 512 + 100), ((LO_B + 401) * 512, (LO_B + 401) * 512 + 100)]))
    rng = np.random.default_rng(nbk)
    made = []
    for i in range(800):
        g = int(rng.integers(6))
        kind = i % 12 if i % 12 in (1, 5) else i % 6 if i % 6 in (2, 3, 4) else 0
        start = EARLY + int(rng.integers(0, 100)) if kind in (1, 5) else F(g)[0]
        made.append((B0 if first_base and i == 0 else start, g, kind))
    made.sort(key=lambda q: q[0])
    rows, far_rows = [], []
    for rank, (start, g, kind) in enumerate(made):                # (every sixteenth read in coordinate order: no tile without one)
        is_far = rank % 16 == 5
        ex = [list(x) for x in isos[g + (6 if is_far else 0)]]
        ex[0][0] = start
        if is_far:
            kind = 2 if (rank // 16) % 4 == 3 else 0
            far_rows.append(rank)
        if kind == 2:
            ex[1][1] -= 5
        elif kind == 3:
            del ex[1]
        elif kind == 4:
            ex[0][1] += 4
            for q in ex[1:-1]:
                q[0] += 4; q[1] += 4
            ex[-1][0] += 4
        elif kind == 5:
            ex = [[start, ex[-1][1]]]
        if not (is_far and last_base):
            ex[-1][1] -= int(rng.integers(0, 40))
        rows.append(_chain([tuple(x) for x in ex]))
    rows, at = _finish(rows)
    return Case(_span_name(nbk, first_base, last_base, dis), "span", txs, rows, dict(ss_dis=dis), (3,), dict(nbk=nbk, far=sorted(at[i] for i in far_rows), far_tx=list(range(6, 12)), far_exon=far))


def span_cases():
    kws = [dict(nbk=383), dict(nbk=384), dict(nbk=385), dict(nbk=384, first_base=True), dict(nbk=384, first_base=True, dis=1),
           dict(nbk=384, last_base=True), dict(nbk=384, last_base=True, dis=1)]
    return [_spec(_span_name(**kw), span_case, **kw) for kw in kws]


# ---- case 4: the window scan

def scan_case(scanned):
    """A transcript over the whole chromosome at the head of the file pins the cursor at 0; behind it short transcripts that end before
    the locus, ten isoforms, and the transcript behind the span as the `scanned`-th one the scan looks at."""
    isos = [_isoform(i) for i in range(10)]
    txs = [(0, 0, [(1_000, 1_200), (300_000, 300_300)])]
    for k in range(scanned - 12):
        txs.append((0, k & 1, [(2_000 + 8 * k, 2_004 + 8 * k)] if k % 7 else [(2_000 + 8 * k, 2_001 + 8 * k), (2_003 + 8 * k, 2_004 + 8 * k)]))
    txs += [(0, i & 1, _with_p(i, ex)) for i, ex in enumerate(isos)] + [STOP]
    rows, kinds = _locus_rows(isos, 800, scanned, isos[-1])
    rows, at = _finish(rows)
    return Case("scan_%d" % scanned, "scan", txs, rows, dict(ss_dis=0), (3,), dict(scanned=scanned, n_win=11, kinds={k: [at[i] for i in v] for k, v in kinds.items()}))


def scan_cases():
    return [_spec("scan_%d" % n, scan_case, n) for n in (WIN_SCAN, WIN_SCAN + 1)]


# ---- case 5: -d

def dis_case(d):
    return window_case(20, dis=d, levels=(3,), name="dis_%d" % d)._replace(family="dis")


def dis_cases():
    return [_spec("dis_%d" % d, dis_case, d) for d in (DIS_MASK_MAX, DIS_MASK_MAX + 1)]


# ---- case 6: the staged positions

def _empty_exon_read(pos, n_exons):
    """A read of n_exons exons under -e 0 and two under -e 1: 10M, n_exons - 1 times 5N back to back (an empty exon between two), 20M."""
    return pos, [(10, M)] + [(5, N_)] * (n_exons - 1) + [(20, M)]


def positions_case(total):
    """Tile 0: 256 reads of 9 or 10 exons under -e 0, and one read that brings the tile's exons to `total`; tile 1: the same at
    TILE_POS_CAP - 1; tile 2: 200 ordinary reads of three exons.  The upload cuts tiles by (ops + 3) / 2 per read: 256 reads of 12 operations
    are 1792, far below the cap, although they have 2300 exons and more."""
    txs = [(0, 0, [(1_000, 1_100), (1_200, 1_300), (1_400, 1_500), (1_600, 1_700)])]
    rows = []
    for t, want in enumerate((total, TILE_POS_CAP - 1)):
        base = min((TILE_POS_CAP - 1, SLAB_POS_CAP - 1), key=lambda c: abs(c - want))
        tens = base - 9 * 255 - 15                               # reads of ten exons; the varied read has 15 + (0 .. 2)
        counts = [10] * tens + [9] * (255 - tens) + [15 + want - base]
        assert sum(counts) == want and len(counts) == 256 and 0 <= tens <= 255
        for k, n in enumerate(counts):
            rows.append(_empty_exon_read(900 + 3 * t + k % 3, n))
    iso = txs[0][2]
    for k in range(200):
        ex = [list(x) for x in iso[k % 2:]]
        ex[0][0] = 1_000 + k % 50 if k % 2 == 0 else ex[0][0]
        if k % 5 == 3:
            ex[1][1] -= 7
        if k % 5 == 4:
            for q in ex:
                q[0] += 9; q[1] += 9
        rows.append(_chain([tuple(x) for x in ex]))
    rows = [(0, p, i & 1, ops) for i, (p, ops) in enumerate(sorted(rows, key=lambda r: r[0]))]
    return Case("pos_%d" % total, "positions", txs, rows, dict(ss_dis=0, min_exon=0), (3,), dict(total=total))


def positions_cases():
    return [_spec("pos_%d" % (c + d), positions_case, c + d) for c in (TILE_POS_CAP, SLAB_POS_CAP) for d in (-1, 0, 1)]


# ---- case 7: the rows of a slab column, the exon-count byte

def rows_case(counts, name, annotated=True):
    """Four tiles of ordinary three-exon reads; in the middle of tile t one read that copies a whole transcript of counts[t] exons, from its
    second exon on (an acceptor: the read is known, and its last exon is the transcript's).  Such a transcript puts its exons into the
    START slice of its tile: from 169 exons on the tile is the chunked kernels'.  annotated=False leaves the long transcripts out of the
    annotation: the tiles stay on the 32-bit masks, and only the exon count of their longest read tells them apart."""
    txs, rows = [], []
    for t, n in enumerate(counts):
        base = 10_000 + 40_000 * t
        short = [(base + 100 * k, base + 100 * k + 40) for k in range(4)]
        long_ = [(base + 1_000, base + 1_040)] + [(base + 1_200 + 100 * k, base + 1_240 + 100 * k) for k in range(n)]
        tail = [(base + 1_250 + 100 * k, base + 1_270 + 100 * k) for k in range(3)]
        txs += [(0, 0, short)] + ([(0, 1, long_)] if annotated else []) + [(0, 0, tail)]
        for k in range(228 if t < 3 else 100):
            ex = [list(x) for x in short[1:]]
            if k % 4 == 1:
                ex[0][0] -= 1 + k % 30
            elif k % 4 == 2:
                ex[0][1] += 3
            elif k % 4 == 3:
                ex[0][0] += 3; ex[0][1] += 3; ex[1][0] += 3; ex[1][1] += 3; ex[2][0] += 3
            ex[-1][1] -= k % 20
            rows.append(_chain([tuple(x) for x in ex]))
            if k == 60:
                rows.append(_chain(long_[1:]))
            if k % 20 == 0:                                        # (neighbours behind the long read too)
                rows.append(_chain([tail[0], tail[1], (tail[2][0], tail[2][1] - k % 7)]))
    order = sorted(range(len(rows)), key=lambda i: rows[i][0])
    rows = [(0, rows[i][0], j & 1, rows[i][1]) for j, i in enumerate(order)]
    return Case(name, "rows", txs, rows, dict(ss_dis=0), (3,), dict(counts=counts, long_tx=[3 * t + 1 for t in range(len(counts))] if annotated else None))


def rows_cases():
    return [_spec("rows_slab", rows_case, (23, 24, 25, 26), "rows_slab"), _spec("rows_count_byte", rows_case, (253, 254, 255, 256), "rows_count_byte"),
            _spec("rows_count_byte_novel", rows_case, (253, 254, 255, 256), "rows_count_byte_novel", annotated=False)]


FAMILIES = dict(window=window_cases, slice=slice_cases, span=span_cases, scan=scan_cases, dis=dis_cases, positions=positions_cases, rows=rows_cases)
_made = {}


def names(family):
    """The names of a family's cases, without building one: the parametrisation of the tests."""
    return [name for name, _build in FAMILIES[family]()]


def case(family, name):
    """One case, built when it is first asked for."""
    if (family, name) not in _made:
        build = dict(FAMILIES[family]())[name]
        _made[family, name] = build()
        assert _made[family, name].name == name and _made[family, name].family == family
    return _made[family, name]


def cases(family):
    return [case(family, name) for name in names(family)]
