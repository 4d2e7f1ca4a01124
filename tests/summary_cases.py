"""The cases of the read classes and unique counts (l2r_summary_*), shared by tests/test_summary_cpu.py and tests/test_gpu_summary.py: the
smallest at which the host routine or the kernels can go wrong.  A case is (reads, options); a read is (tid, info bits, [(start, end),
...]); the options are those of tests/uniq_restatement.merge (s, d, D, f)."""
import itertools

import numpy as np

from tests import uniq_cases as uc
from tests.summary_restatement import FULL, KNOWN, KNOWN_SITE, REV, UNREL

TILE = 256                                                      # SUM_TILE: reads of one tile of the partition
BITS_OF_CLASS = (KNOWN, KNOWN_SITE, KNOWN_SITE | UNREL, 0)


def with_classes(trans, classes):
    """Transcripts (tid, rev, chain) as reads of the given classes."""
    return [(tid, BITS_OF_CLASS[c] | (REV if rev else 0), chain) for (tid, rev, chain), c in zip(trans, classes)]


def bit_combinations():
    """(reads, the class of every read by hand): all eight combinations of KNOWN / KNOWN_SITE / UNREL, with FULL clear and set; every read
    a cluster of its own."""
    reads, want = [], []
    by_hand = {(0, 0, 0): 3, (0, 0, 1): 3, (0, 1, 0): 1, (0, 1, 1): 2, (1, 0, 0): 0, (1, 0, 1): 0, (1, 1, 0): 0, (1, 1, 1): 0}
    for i, (full, known, site, unrel) in enumerate(itertools.product((0, 1), repeat=4)):
        bits = (KNOWN if known else 0) | (KNOWN_SITE if site else 0) | (UNREL if unrel else 0) | (FULL if full else 0)
        reads.append((0, bits, [(1000 * i + 1, 1000 * i + 100), (1000 * i + 200, 1000 * i + 300)]))
        want.append(by_hand[(known, site, unrel)])
    return reads, want


def twins(c1, c2):
    """Two identical chains, in classes c1 and c2."""
    chain = [(100, 200), (300, 400)]
    return with_classes([(0, 0, chain), (0, 0, chain)], [c1, c2])


def cycling(n, classes=(0, 1, 2, 3)):
    """n reads of uc.loci with classes cycling through `classes`."""
    trans = uc.loci(np.random.default_rng(11), n + 40)[:n]
    return with_classes(trans, [classes[i % len(classes)] for i in range(len(trans))])


def long_chains(k):
    """Six reads of k exons each on two chromosomes, classes 0 0 1 0 1 3: the second is the first again, the fourth differs in an inner
    boundary (or, with one exon, lies elsewhere), the fifth is the third again."""
    def chain(base, bump=0):
        c = [[base + 100 * j, base + 100 * j + 50] for j in range(k)]
        if k > 1:
            c[k // 2][0] += bump
        return [tuple(e) for e in c]
    a, b, d = chain(1000), chain(1010 if k > 1 else 100000, 7), chain(500)
    return with_classes([(0, 0, a), (0, 0, a), (0, 0, a), (0, 0, b), (0, 0, a), (1, 1, d)], [0, 0, 1, 0, 1, 3])


def one_cluster(n):
    """n identical reads of one class."""
    return with_classes([(0, 0, [(100, 200), (300, 400)])] * n, [1] * n)


def descends_overall():
    """Class 0 on chromosome 1, then class 1 on chromosome 0: (tid, start) descends over the input, but inside no class."""
    a = [(1, 0, [(100 + 10 * i, 200 + 10 * i), (900, 950)]) for i in range(5)]
    b = [(0, 0, [(100 + 10 * i, 200 + 10 * i), (900, 950)]) for i in range(5)]
    return with_classes(a + b, [0] * 5 + [1] * 5)


def descends_in_a_class():
    reads = descends_overall()
    return reads + [reads[0]]                                   # class 0 again, at its first start


def edge_cases():
    """name -> (reads, the text of the refusal or None)."""
    one = [(100, 200), (300, 400)]
    return {
        "tid_top": ([((1 << 29) - 1, KNOWN, one)], None),
        "tid_beyond": ([(0, KNOWN, one), (1 << 29, KNOWN, one)], "read 1: a tid outside [0, 2^29)"),
        "tid_negative": ([(-1, 0, one)], "read 0: a tid outside [0, 2^29)"),
        "no_exon": ([(0, KNOWN, one), (0, KNOWN_SITE, one), (0, 0, [])], "read 2: no exon"),
        "coordinate_0": ([(0, 0, [(0, 5)])], None),
        "coordinate_negative": ([(0, 0, one), (0, 0, [(-1, 5), (7, 9)])], "read 1: a negative coordinate"),
        "smallest_read_first": ([(0, 0, one), (0, 0, [(3, 5), (-7, 9)]), (1 << 29, 0, one), (0, 0, [])], "read 1: a negative coordinate"),
    }


GENERATED_SEED = 1                                            # chosen on the CPU: tests/test_summary_cpu.py asserts what the set must hold
GENERATED_OPTS = uc.GENERATED_OPTS


def generated():
    """uc.loci with classes drawn 60 / 20 / 10 / 10, one draw for every eight reads in a row: a locus's reads mostly share a class, as a
    gene's do, so that the small classes see hits of every kind too."""
    rng = np.random.default_rng(GENERATED_SEED)
    trans = uc.loci(rng, 2000)
    return with_classes(trans, np.repeat(rng.choice(4, size=len(trans) // 8 + 1, p=[0.6, 0.2, 0.1, 0.1]), 8)[:len(trans)])


def cases():
    """name -> (reads, options): the sound cases, which both routes and the restatement answer alike."""
    c = {"n0": ([], {}), "bits": (bit_combinations()[0], {})}
    c["twins_two_classes"] = (twins(0, 1), {})
    c["twins_one_class"] = (twins(2, 2), {})
    for name, (reads, refusal) in edge_cases().items():
        if refusal is None:
            c[name] = (reads, {})
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        c["cycling_%d" % n] = (cycling(n), GENERATED_OPTS)
    c["one_class_absent"] = (cycling(300, (0, 1, 3)), GENERATED_OPTS)
    c["all_one_class"] = (cycling(300, (2,)), GENERATED_OPTS)
    for k in (1, 63, 64, 65, 200):
        c["chains_%d" % k] = (long_chains(k), dict(f=0.5))
    c["descends_overall"] = (descends_overall(), {})
    c["generated"] = (generated(), GENERATED_OPTS)
    return c
