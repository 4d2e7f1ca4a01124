"""The cases of merge_trans over a list of transcripts (l2r_uniq_merge), shared by tests/test_uniq_cpu.py and tests/test_gpu_uniq.py: the
smallest at which the host routine or the kernels can go wrong.  A case is (transcripts, options); a transcript is (tid, rev, [(start,
end), ...]); the options are those of tests/uniq_restatement.merge (s, d, D, f).  The cases beyond three tiles of the prefix maximum
(the second half of this file) come as columns where they are large, and with the answer they are built to give."""
import numpy as np

TILE = 256                                                      # L2R_UNIQ_PMAX_TILE (asserted in tests/test_uniq_cpu.py)


def ladder(k, base=1000):
    """k transcripts of two exons that overlap each other and never match (-d 0): one cluster whose list holds k entries."""
    return [(0, 0, [(base + j, base + 1000 + 2 * j), (base + 4000 + 2 * j, base + 8000)]) for j in range(k)]


def ladder_hit(k, j, base=1000):
    """An offer behind ladder(k) that is identical to its entry j alone (its first start is free under the default -D)."""
    return (0, 0, [(base + k, base + 1000 + 2 * j), (base + 4000 + 2 * j, base + 8000)])


def lane_round_case(k):
    """A list of k entries, then hits on the oldest entry, on entries 63 and 64 where the list has them, and on the newest."""
    targets = sorted({0, k - 1} | {j for j in (63, 64) if j < k})
    return ladder(k) + [ladder_hit(k, j) for j in targets], targets


def scattered(n):
    """n transcripts, every one a cluster of its own."""
    return [(0, i & 1, [(1000 * i + 1, 1000 * i + 100), (1000 * i + 200, 1000 * i + 300)]) for i in range(n)]


def loci(rng, n, n_chrom=3, spread=400, gaps=True):
    """About n transcripts over n_chrom chromosomes, in (tid, start) order: loci of a few isoforms each, read as jittered duplicates,
    as prefixes and suffixes of a chain, and as single-exon reads.  Without gaps every locus overlaps the next."""
    out = []
    per_chrom = max(1, n // n_chrom)
    for tid in range(n_chrom):
        made, pos = 0, 1000
        while made < per_chrom:
            n_iso = int(rng.integers(1, 4))
            isoforms = []
            for _ in range(n_iso):
                k = int(rng.integers(2, 7))
                cuts = np.sort(rng.choice(np.arange(pos, pos + spread * k, 10), 2 * k, replace=False))
                isoforms.append([(int(cuts[2 * q]), int(cuts[2 * q + 1])) for q in range(k)])
            for _ in range(int(rng.integers(3, 14))):
                kind = int(rng.integers(0, 10))
                iso = isoforms[int(rng.integers(0, n_iso))]
                rev = int(rng.integers(0, 8) == 0)
                if kind < 5:                                    # a duplicate: ends moved freely, inner boundaries by 0..3
                    ch = [[s + int(rng.integers(-1, 3)), e + int(rng.integers(-1, 3))] for s, e in iso]
                    ch[0][0] = iso[0][0] + int(rng.integers(-8, 30)); ch[-1][1] = iso[-1][1] + int(rng.integers(-30, 30))
                elif kind < 8 and len(iso) > 2:                 # a prefix or a suffix of the chain
                    m = int(rng.integers(2, len(iso)))
                    ch = [list(e) for e in (iso[:m] if kind & 1 else iso[-m:])]
                    ch[0][0] += int(rng.integers(0, 5)); ch[-1][1] -= int(rng.integers(0, 5))
                else:                                           # a single-exon read
                    s = iso[0][0] + int(rng.integers(0, 40))
                    ch = [[s, s + int(rng.integers(150, 260))]]
                ch = [(max(1, s), max(max(1, s), e)) for s, e in ch]
                out.append((tid, rev, ch))
                made += 1
            pos += spread * 7 if rng.integers(0, 4) and gaps else spread # mostly a gap behind a locus, now and then the next one overlaps
    out.sort(key=lambda t: (t[0], t[2][0][0]))
    return out[:n] if len(out) > n else out


GENERATED_SEED = 5                                              # chosen on the CPU: tests/test_uniq_cpu.py asserts what the set must hold
GENERATED_OPTS = dict(s=0, d=2, D=40, f=0.8)


def generated():
    return loci(np.random.default_rng(GENERATED_SEED), 2000)


def fraction_case():
    """Two single-exon reads whose overlap fraction is 2 / 3: -f exactly there, one ulp above (no hit) and one below."""
    trans = [(0, 0, [(100, 102)]), (0, 0, [(101, 103)])]
    r = np.float32(np.float64(2) / np.float64(3))
    return trans, r, np.nextafter(r, np.float32(2)), np.nextafter(r, np.float32(0))


def cases():
    """name -> (transcripts, options)."""
    c = {}
    one = (0, 0, [(100, 200), (300, 400)])
    c["n0"] = ([], {})
    c["n1"] = ([one], {})
    c["n1_single"] = ([(2, 1, [(5, 9)])], {})
    # start equal to the running maximum end: the same cluster; one above it: a new one
    c["cluster_edge"] = ([(0, 0, [(100, 150), (180, 500)]), (0, 0, [(120, 130), (140, 160)]), (0, 0, [(500, 600), (700, 800)]),
                          (0, 0, [(801, 900), (950, 990)]), (0, 0, [(990, 995), (997, 999)])], {})
    # the same chains on two chromosomes: nothing merges across, although the coordinates overlap
    c["chromosome_change"] = ([(0, 0, [(100, 200), (300, 400)]), (0, 0, [(100, 200), (300, 400)]), (1, 0, [(100, 200), (300, 400)]),
                               (1, 0, [(150, 200), (300, 400)]), (2, 0, [(1, 2)])], {})
    # mutation carried forward: the second offer raises the entry's end 400 -> 700, the third starts between the two and merges only
    # because the scan does not stop at 400, the fourth is within -D of the end only once that is 700
    c["mutation_forward"] = ([(0, 0, [(100, 400)]), (0, 0, [(105, 700)]), (0, 0, [(420, 700)]), (0, 0, [(425, 1030)])], dict(D=330, f=0.4))
    c["mutation_forward_multi"] = ([(0, 0, [(100, 200), (300, 400)]), (0, 0, [(100, 200), (300, 450)]), (0, 0, [(420, 430), (440, 445)]),
                                    (0, 0, [(421, 430), (440, 447)])], dict(D=10000))
    # early stop: the list holds a long entry, then a short one; the offer starts beyond the short one's end and matches the long one
    c["early_stop"] = ([(0, 0, [(100, 200), (300, 1000)]), (0, 0, [(150, 160), (170, 180)]), (0, 0, [(185, 200), (300, 1000)])], {})
    # -s: an entry of the other strand, identical to the offer, between the offer and its match
    c["strand_between"] = ([(0, 0, [(100, 200), (300, 400)]), (0, 1, [(100, 200), (300, 400)]), (0, 0, [(100, 200), (300, 400)]),
                            (0, 1, [(100, 300)]), (0, 0, [(100, 300)]), (0, 1, [(100, 300)])], dict(s=1))
    c["strand_free"] = (c["strand_between"][0], dict(s=0))
    # mixed exon counts: single offered to multi and multi to single take neither branch
    c["mixed_counts"] = ([(0, 0, [(100, 400)]), (0, 0, [(100, 200), (300, 400)]), (0, 0, [(100, 400)]), (0, 0, [(100, 200), (300, 400)]),
                          (0, 0, [(350, 1000)])], {})
    # contained, both directions (the longer offer is dropped: Q8), and two that are not
    c["contained"] = ([(0, 0, [(100, 200), (300, 400), (500, 600)]), (0, 0, [(100, 200), (300, 400)]), (0, 0, [(350, 400), (500, 600)]),
                       (0, 0, [(350, 400), (500, 600), (700, 800)]), (0, 0, [(350, 410), (500, 600)]),
                       (1, 0, [(100, 200), (300, 400)]), (1, 0, [(100, 200), (300, 400), (500, 600)]), (1, 0, [(100, 200), (300, 400), (500, 600), (700, 800)])], {})
    # the walk over the matched introns advances the outer index and breaks: the first place that fits is the only one tried
    c["inner_walk"] = ([(0, 0, [(100, 200), (300, 400), (500, 600), (700, 800), (900, 1000)]), (0, 0, [(150, 202), (298, 400), (500, 600), (700, 1000)]),
                        (0, 0, [(150, 400), (500, 600), (700, 800), (900, 1000)]), (0, 0, [(160, 200), (300, 400), (500, 611)])], dict(d=2))
    # ... here the shorter chain's first intron fits the longer one's introns 0 and 1 (-d 2); from 0 the walk fails, from 1 it would not
    c["inner_walk_first_fit"] = ([(0, 0, [(100, 200), (203, 204), (207, 300), (400, 500)]), (0, 0, [(150, 202), (205, 300), (400, 500)])], dict(d=2))
    # -D and -d: at the distance and one beyond
    for name, D, d in (("D_at", 50, 0), ("D_beyond", 49, 0), ("d_at", 1000, 3), ("d_beyond", 1000, 2)):
        c[name] = ([(0, 0, [(100, 200), (300, 400), (500, 600)]), (0, 0, [(150, 200), (300, 400), (500, 650)]), (0, 0, [(150, 203), (297, 400), (500, 600)]),
                    (0, 0, [(150, 300)]), (0, 0, [(200, 350)])], dict(D=D, d=d, f=0.1))
    for k in (64, 65, 128, 129):
        c["lanes_%d" % k] = (lane_round_case(k)[0], {})
    c["own_clusters"] = (scattered(2 * TILE + 1), {})
    c["one_cluster"] = (ladder(300) + [ladder_hit(300, 7), ladder_hit(300, 299)], {})
    return c


def tile_cases():
    """n at the prefix maximum's tile size minus one, at it, plus one, and at two tiles plus one: prefixes of one generated set."""
    base = loci(np.random.default_rng(11), 2 * TILE + 40)
    return {"tile_%d" % n: (base[:n], GENERATED_OPTS) for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)}


def unsorted_case():
    """Loci in descending order of their chromosomes and a swap inside one: not in (tid, start) order."""
    base = loci(np.random.default_rng(3), 120)
    return base[::-1][:60] + base[:60], GENERATED_OPTS


# ---------------------------------------------------------------------------------------------------- beyond three tiles
WAVE = 64 * TILE                                                # transcripts of one wave of k_uniq_pmax
ROUND = 1024 * TILE                                             # ... and of one of its rounds
N_TAIL = TILE + 3


def reach_columns(p, r, n_tail=N_TAIL, tid=0, tid_behind=None, long_end=None, spacing=100):
    """Columns (tid, rev, ex_off, xs, xe) of r + 1 + n_tail transcripts of two exons, transcript i at spacing * i + 1, 31 bases long
    and so a cluster of its own -- but transcript p, which ends where transcript r starts (or at long_end): p .. r are one cluster,
    whose members never match (-d 0) and whose every offer stops at the entry in front of it.  tid_behind: the chromosome of the
    transcripts behind p, which are then clusters of their own again."""
    n = r + 1 + n_tail
    s = np.arange(n, dtype=np.int64) * spacing + 1
    xs, xe = np.empty(2 * n, np.int64), np.empty(2 * n, np.int64)
    xs[0::2], xe[0::2], xs[1::2], xe[1::2] = s, s + 10, s + 20, s + 30
    xe[2 * p + 1] = s[r] if long_end is None else long_end
    t = np.full(n, tid, np.int64)
    if tid_behind is not None:
        t[p + 1:] = tid_behind
    assert xs.max() < 2 ** 31 and xe.max() < 2 ** 31 and (xs <= xe).all()
    return t.astype(np.int32), np.zeros(n, np.uint8), 2 * np.arange(n + 1, dtype=np.int64), xs.astype(np.int32), xe.astype(np.int32)


def reach_expected(p, r, n):
    """head flags, clusters, largest cluster of reach_columns(p, r) on one chromosome: nothing merges, so unique = n."""
    head = np.ones(n, np.uint8)
    head[p + 1:r + 1] = 0
    return head, n - (r - p), r - p + 1


REACH_PAIRS = [(0, 1), (62, 63), (63, 64), (0, TILE - 1),                                               # inside a tile, at its wave edges
               (TILE - 1, TILE), (0, TILE), (0, TILE + 1),                                              # tile edge
               (3, 2 * TILE + 5), (TILE - 1, 3 * TILE),                                                 # through a whole tile whose own maximum is smaller
               (5, WAVE - 6), (5, WAVE), (5, WAVE + 1), (WAVE - 1, WAVE), (WAVE - 1, WAVE + TILE + 3),  # wave edge of the prefix maximum
               (ROUND - 1, ROUND + 300),                                                                # round edge, a small cluster
               (ROUND + WAVE - 1, ROUND + WAVE + 5)]                                                    # wave edge inside the second round
REACH_ROUND_PAIRS = [(5, ROUND), (5, ROUND + TILE + 7)]         # one cluster across the round edge: 262 k offers through one wave

# the long transcript at the last slot of a wave inside a tile, of a tile, of a wave of k_uniq_pmax and of a round; what follows it lies
# on the next chromosome and starts below its end
STEP_SLOTS = [63, TILE - 1, WAVE - 1, ROUND - 1]
STEP_CHROMS = [(-1, 0), (0, 1), (2147483646, 2147483647)]
STEP_ENDS = [None, 2147483646]


def step_columns(p, chroms, long_end):
    return reach_columns(p, p + N_TAIL, n_tail=0, tid=chroms[0], tid_behind=chroms[1], long_end=long_end)


def deep_mutation_case(k, j, base=1000):
    """ladder(k), then four offers identical to its entry j alone whose ends lie 250, 500, 750 and 1300 above the ladder's, under
    -D 300: the second and the third merge only because the one before raised the entry's end; the fourth is pushed."""
    offers = [(0, 0, [(base + k, base + 1000 + 2 * j), (base + 4000 + 2 * j, base + 8000 + up)]) for up in (250, 500, 750, 1300)]
    return ladder(k, base) + offers, dict(D=300)


DEEP_MUTATION = [(65, 0), (129, 0), (129, 64), (129, 65), (200, 0), (200, 71), (200, 72), (200, 135), (200, 136), (200, 199)]


def stop_hit_case(n_fill, hit):
    """-s 1.  Two entries of strand +, a long chain and a short one that ends before the offer starts; n_fill entries of strand - that
    overlap everything and never match each other; an offer of strand + identical to the long chain.  The fillers are skipped.  With
    the short entry the newer of the two (hit = False) it stops the scan and the offer is pushed although the long entry matches; with
    the long one the newer (hit = True) the offer merges into it (entry 1)."""
    long_ = (0, 0, [(100, 2000), (3000, 10000)])
    pair = [(0, 0, [(50, 60), (70, 150)]), long_] if hit else [long_, (0, 0, [(150, 160), (170, 180)])]
    fill = [(0, 1, [(181 + i, 5000 + 2 * i), (6000 + 2 * i, 20000)]) for i in range(n_fill)]
    return pair + fill + [(0, 0, [(400, 2000), (3000, 10000)])], dict(s=1)


STOP_HIT_FILL = [0, 61, 62, 63, 64, 126, 127, 128]


def two_hits_case(k, j, base=1000):
    """ladder(k) under -d 1 and an offer whose inner boundaries lie between those of the entries j and j + 1: identical to both, and
    the newer one, j + 1, takes it."""
    return ladder(k, base) + [(0, 0, [(base + k, base + 1001 + 2 * j), (base + 4001 + 2 * j, base + 8000)])], dict(d=1)


TWO_HITS = [(70, 3), (70, 5), (130, 64), (130, 65)]


def several_rounds_case(c):
    """lane_round_case(65) on each of c chromosomes: c clusters of more than one lane round."""
    one = lane_round_case(65)[0]
    return [(tid, rev, chain) for tid in range(c) for _t, rev, chain in one], {}


SEVERAL = [3, 4, 5, 9]                                          # (UNIQ_WAVES = 4: a full workgroup, and a last one that is partly filled)


def walk_cases():
    """name -> (transcripts, options, the literal answer: merged and uniq_of of the offers behind the lists)."""
    c = {}
    for k, j in DEEP_MUTATION:
        c["deep_mutation_%d_%d" % (k, j)] = deep_mutation_case(k, j) + (([1, 1, 1, 0], [j, j, j, k]),)
    for n_fill in STOP_HIT_FILL:
        c["stop_over_hit_%d" % n_fill] = stop_hit_case(n_fill, False) + (([0], [n_fill + 2]),)
        c["hit_over_stop_%d" % n_fill] = stop_hit_case(n_fill, True) + (([1], [1]),)
    for k, j in TWO_HITS:
        c["two_hits_%d_%d" % (k, j)] = two_hits_case(k, j) + (([1], [j + 1]),)
    for n in SEVERAL:
        targets = lane_round_case(65)[1]
        c["several_rounds_%d" % n] = several_rounds_case(n) + (([1] * len(targets), [65 * (n - 1) + j for j in targets]),)
    return c


DENSE_SEED, DENSE_N = 5, 20000                                  # chosen on the CPU: tests/test_uniq_cpu.py asserts what the sets must hold
# (the generator makes a cluster per 10 transcripts or so: 70 000 of them are 6 815 clusters, 180 000 are 17 492)
WIDE_SEED, WIDE_N = 5, 180000
_SETS = {}


def _made(which, rng_seed, n, gaps):
    if which not in _SETS:
        from tests import uniq_restatement as ur
        trans = loci(np.random.default_rng(rng_seed), n, gaps=gaps)
        _SETS[which] = (trans, ur.columns(trans))
    return _SETS[which]


def dense():
    """(transcripts, their columns).  Every locus overlaps the next: a few clusters whose lists run to thousands of entries."""
    return _made("dense", DENSE_SEED, DENSE_N, False)


def wide():
    """(transcripts, their columns) of generated()'s generator: more clusters than one round of the scan over their list lengths
    holds (16 384), and more transcripts than one wave of k_uniq_pmax."""
    return _made("wide", WIDE_SEED, WIDE_N, True)
