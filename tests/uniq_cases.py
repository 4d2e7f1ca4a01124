"""The cases of merge_trans over a list of transcripts (l2r_uniq_merge), shared by tests/test_uniq_cpu.py and tests/test_gpu_uniq.py: the
smallest at which the host routine or the kernels can go wrong.  A case is (transcripts, options); a transcript is (tid, rev, [(start,
end), ...]); the options are those of tests/uniq_restatement.merge (s, d, D, f)."""
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


def loci(rng, n, n_chrom=3, spread=400):
    """About n transcripts over n_chrom chromosomes, in (tid, start) order: loci of a few isoforms each, read as jittered duplicates,
    as prefixes and suffixes of a chain, and as single-exon reads."""
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
            pos += spread * 7 if rng.integers(0, 4) else spread          # mostly a gap behind a locus, now and then the next one overlaps
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
