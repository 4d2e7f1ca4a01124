"""Cases for the novel list of `update-gtf` (l2r_novel_*): tests/test_novel_cpu.py runs them through novel_host, tests/test_gpu_novel.py
through both routes of the engine.  A read is (tid, info bits, ref, [(start, end, flags), ...]) as in tests/novel_restatement.py; a case
is (reads, opts) with opts = the keyword arguments of novel_restatement.novel beside ref_names."""
import numpy as np

from tests import novel_restatement as nr

REFS = [b"chr1", b"chr2", b"chrX"]
OFFER = nr.FULL | nr.KNOWN_SITE                 # an offer where no junction table is set
TX_GENE = [0, 0, 1, 2, 2, 3]                    # six annotation transcripts of four genes
BASE = dict(tx_gene=TX_GENE, na_gene=4)         # no annotation gene is called NA: NA takes the next ordinal


def chain(start, k, flags=0, step=100, width=50):
    """k exons from `start` on, every one with `flags` (an int, or a function of j)."""
    return [(start + j * step, start + j * step + width, flags(j) if callable(flags) else flags) for j in range(k)]


def mixed(n, seed=5):
    """n reads on three chromosomes in order: offers (some twice, so that there are hits), known reads, and others; offers at the wave
    and tile edges."""
    rng = np.random.default_rng(seed)
    reads = []
    edges = {0, 62, 63, 64, 65, 254, 255, 256, 257, n - 1}
    for i in range(n):
        tid = 0 if i < n // 2 else 1 if i < n - n // 8 else 2
        start = 1000 + 300 * i
        k = int(rng.integers(1, 6))
        ch = [(start + 40 * j, start + 40 * j + 20, int(rng.integers(0, 16))) for j in range(k)]
        what = int(rng.integers(0, 4))
        if i in edges or what == 0:
            reads.append((tid, OFFER | (nr.REV if i % 3 == 0 else 0), int(rng.integers(-1, len(TX_GENE))), ch))
            if i % 4 == 0 and i not in edges:
                reads[-1] = (tid, OFFER, 1, ch)
        elif what == 1:
            reads.append((tid, nr.KNOWN | (nr.FULL if i % 2 else 0), int(rng.integers(0, len(TX_GENE))), ch))
        else:
            reads.append((tid, nr.FULL if what == 2 else nr.KNOWN_SITE, -1, ch))
    return reads


def twice(reads):
    """Every offer a second time right behind itself: identical hits, coverage 2."""
    out = []
    for r in reads:
        out.append(r)
        if nr.is_offer(r[1], 0):
            out.append(r)
    return out


def bit_combinations():
    """Every combination of FULL, KNOWN, KNOWN_SITE and SJ_PASS, in order on one chromosome."""
    reads = []
    for v in range(16):
        bits = (nr.FULL if v & 1 else 0) | (nr.KNOWN if v & 2 else 0) | (nr.KNOWN_SITE if v & 4 else 0) | (nr.SJ_PASS if v & 8 else 0)
        reads.append((0, bits, v % len(TX_GENE), chain(1000 * (v + 1), 2, nr.NE | nr.NJ)))
    return reads


def long_chains(k):
    """Three offers of k exons -- the second repeats the first with a longer last exon: an identical hit that widens the end, whose last
    exon is novel -- and one of two exons."""
    f = lambda j: (nr.NE if j in (0, k - 1, k // 2) else 0) | (nr.ND | nr.NA | nr.NJ if j % 2 == 0 else 0)
    a = chain(1000, k, f)
    b = a[:-1] + [(a[-1][0], a[-1][1] + 7, a[-1][2])]
    return [(0, OFFER, 0, a), (0, OFFER, 0, b), (0, OFFER, 2, chain(1000 + 100 * k + 500, k, f)), (1, OFFER | nr.REV, -1, chain(50, 2, nr.NE))]


def widened_end():
    """... on the device route: the BED must show the widened end of the novel last exon (a composer that reads the source's chain fails)."""
    return [(0, OFFER, 0, [(100, 200, 0), (300, 400, nr.NE)]), (0, OFFER, 0, [(100, 200, 0), (300, 450, nr.NE)])]


def widened_start():
    """A later offer with a smaller start: the input descends (the host routine), the identical hit lowers the entry's start, and the novel
    first exon shows it."""
    return [(0, OFFER, 0, [(100, 200, nr.NE), (300, 400, 0)]), (0, OFFER, 0, [(90, 200, nr.NE), (300, 400, 0)])]


def contained_hit():
    """The shorter chain lies in the longer one: merged, nothing changes (coverage 1, ends as they were)."""
    return [(0, OFFER, 0, [(100, 200, nr.NE), (300, 400, nr.NJ), (500, 600, 0)]), (0, OFFER, 0, [(100, 200, 0), (300, 410, nr.NE)])]


def single_exon_hit():
    return [(0, OFFER, -1, [(100, 200, nr.NE)]), (0, OFFER, -1, [(100, 210, nr.NE)]), (0, OFFER, -1, [(5000, 5100, 0)])]


def opposite_strands():
    """With -c the second offer does not merge with the first."""
    return [(0, OFFER, 0, [(100, 200, nr.NE), (300, 400, 0)]), (0, OFFER | nr.REV, 0, [(100, 200, nr.NE), (300, 400, 0)])]


def inner_then_terminal():
    """The same exon as I in its first entry and T in a later one on the other strand: the first wins, the score is both coverages (the
    later entry is there twice: coverage 2)."""
    second = (0, OFFER | nr.REV, 2, [(300, 400, nr.NE), (700, 800, 0)])
    return [(0, OFFER, 0, [(100, 200, 0), (300, 400, nr.NE), (500, 600, 0)]), second, second]


def two_tids_one_exon():
    return [(0, OFFER, 0, [(100, 200, nr.NE), (300, 400, 0)]), (1, OFFER, 0, [(100, 200, nr.NE), (300, 400, 0)])]


def donor_is_acceptor():
    """One coordinate as a donor and as an acceptor: counted in both lists."""
    return [(0, OFFER, 0, [(100, 200, nr.ND), (200, 300, 0)]), (0, OFFER, 0, [(150, 160, nr.NA), (200, 300, 0), (400, 500, 0)])]


def last_exon_flags():
    """The junction bits of the last exon are ignored, its exon bit is not."""
    return [(0, OFFER, 0, [(100, 200, 0), (300, 400, nr.NE | nr.ND | nr.NA | nr.NJ)]), (1, OFFER, 1, [(100, 200, nr.ND | nr.NA | nr.NJ)])]


def start_zero():
    return [(0, OFFER, -1, [(0, 50, nr.NE)]), (0, OFFER | nr.REV, -1, [(0, 9, nr.NE), (20, 30, nr.NE)])]


def genes():
    """Transcripts 0, 2 and 3 are of genes 0, 1 and 2.  Gene 0 on two chromosomes with other genes between them: counted twice.  Gene 2 the
    newest row when the second chromosome ends and the first on the third: add_gene compares before it stops, counted once.  ref < 0
    twice: once."""
    one = lambda tid, ref, at: (tid, OFFER, ref, [(at, at + 50, 0), (at + 100, at + 150, 0)])
    known = lambda tid, ref, at: (tid, nr.KNOWN, ref, [(at, at + 50, 0)])
    return [one(0, 0, 100), known(0, 0, 150), one(0, 2, 1000), known(0, 2, 1100), one(0, -1, 2000), one(0, -1, 3000),
            one(1, 0, 100), known(1, 0, 150), one(1, 3, 1000), known(1, 3, 1100), one(2, 3, 100), known(2, 3, 150), one(2, 0, 1000), known(2, 0, 1100)]


def gene_called_na():
    """An annotation gene called NA (ordinal 1 here) and ref < 0 are one gene."""
    return [(0, OFFER, 2, [(100, 200, 0), (300, 400, 0)]), (0, OFFER, -1, [(1000, 1100, 0), (1300, 1400, 0)]), (0, nr.KNOWN, 2, [(5, 9, 0)]), (0, nr.KNOWN, -1, [(50, 90, 0)])]


def known_reads(n, per_key):
    """n known reads, `per_key` in a row with one (tid, gene): n items of the known-gene list and nothing else."""
    tx = list(range((n + per_key - 1) // per_key + 1))
    return [(0 if i < n // 2 else 1, nr.KNOWN, i // per_key, [(10 * i, 10 * i + 5, 0)]) for i in range(n)], dict(tx_gene=tx, na_gene=len(tx))


def third_word():
    """Junctions with one donor and different acceptors (keys that differ in the third word alone), and the same junction on two
    chromosomes (in the first alone); -d 0, so nothing merges."""
    return [(0, OFFER, 0, [(100, 200, nr.NJ), (300, 400, 0)]), (0, OFFER, 0, [(150, 200, nr.NJ), (350, 400, 0)]), (0, OFFER, 0, [(160, 200, nr.NJ), (300, 400, 0)]),
            (1, OFFER, 0, [(100, 200, nr.NJ), (300, 400, 0)])]


def descending_offers():
    return [(0, OFFER, 0, [(5000, 5100, nr.NE), (5300, 5400, 0)]), (0, OFFER, 1, [(100, 200, nr.NE), (300, 400, 0)]), (1, OFFER, 2, [(100, 200, nr.NE)])]


def descending_known():
    return [(1, nr.KNOWN, 0, [(100, 200, 0)]), (0, OFFER, 0, [(100, 200, nr.NE), (300, 400, 0)]), (0, nr.KNOWN, 3, [(100, 200, 0)]), (1, OFFER, 0, [(100, 200, nr.NE)])]


def cases():
    out = {"empty": ([], dict(BASE)), "one": ([(1, OFFER | nr.REV, 3, chain(100, 2, nr.NE | nr.ND | nr.NA | nr.NJ))], dict(BASE)),
           "no_offer": ([(0, nr.KNOWN | nr.FULL, 0, chain(100, 2)), (0, nr.FULL, -1, chain(500, 1, nr.NE))], dict(BASE)),
           "known_not_full": ([(0, nr.KNOWN, 5, chain(100, 3, nr.NE))], dict(BASE)),
           "bits_no_sj": (bit_combinations(), dict(BASE)), "bits_sj": (bit_combinations(), dict(BASE, has_sj=1)),
           "widened_end": (widened_end(), dict(BASE, D=100)), "contained": (contained_hit(), dict(BASE, D=1000)),
           "single_exon_hit": (single_exon_hit(), dict(BASE, D=20, f=0.5)), "opposite_strands": (opposite_strands(), dict(BASE, s=1)),
           "same_strands_merge": (opposite_strands(), dict(BASE)),
           "inner_then_terminal": (inner_then_terminal(), dict(BASE, D=10)), "two_tids_one_exon": (two_tids_one_exon(), dict(BASE)),
           "donor_is_acceptor": (donor_is_acceptor(), dict(BASE, D=10)), "last_exon_flags": (last_exon_flags(), dict(BASE)), "start_zero": (start_zero(), dict(BASE)),
           "genes": (genes(), dict(BASE)), "gene_called_na": (gene_called_na(), dict(tx_gene=[0, 0, 1], na_gene=1)),
           "third_word": (third_word(), dict(BASE, D=5)),
           "all_equal": known_reads(300, 300), "all_distinct": known_reads(300, 1)}
    for n in (63, 64, 65, 255, 256, 257):
        out["mixed_%d" % n] = (mixed(n), dict(BASE, D=30))
    out["mixed_twice"] = (twice(mixed(300, 9)), dict(BASE, D=30))
    for n in (4095, 4096, 4097):
        out["items_%d" % n] = known_reads(n, 3)
    return out


def unordered_cases():
    return {"widened_start": (widened_start(), dict(BASE, D=100)), "descending_offers": (descending_offers(), dict(BASE)), "descending_known": (descending_known(), dict(BASE))}


def edge_cases():
    """name -> (reads, opts, refusal or None): every domain error at its edge; the smallest read and the first of its kinds is named."""
    ok = (0, OFFER, 0, chain(100, 2, nr.NE))
    n_tx = len(TX_GENE)
    return {
        "tid_last": ([ok, (2, OFFER, 0, chain(100, 1))], BASE, None),
        "tid_beyond": ([ok, (3, nr.FULL, 0, chain(100, 1))], BASE, "read 1: a tid outside the reference table"),
        "tid_negative": ([(-1, nr.KNOWN, 0, chain(100, 1)), ok], BASE, "read 0: a tid outside the reference table"),
        "no_exon": ([ok, ok, (0, nr.KNOWN, 0, [])], BASE, "read 2: no exon"),
        "ref_last": ([ok, (0, nr.KNOWN, n_tx - 1, chain(900, 1))], BASE, None),
        "ref_beyond": ([ok, (0, nr.KNOWN, n_tx, chain(900, 1))], BASE, "read 1: ref at or beyond the annotation's transcripts"),
        "negative_offer": ([ok, (0, OFFER, 0, [(500, 600, 0), (-700, 800, 0)])], BASE, "read 1: a negative coordinate"),
        "negative_elsewhere": ([ok, (0, nr.KNOWN, 0, [(-5, 600, 0)])], BASE, None),
        "two_kinds": ([ok, (0, OFFER, 0, [(-1, 5, 0)]), (7, OFFER, n_tx, [])], BASE, "read 1: a negative coordinate"),
        "first_kind": ([(7, OFFER, n_tx, [])], BASE, "read 0: a tid outside the reference table"),
    }
