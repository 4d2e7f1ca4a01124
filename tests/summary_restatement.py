"""The read classes and unique counts of `update-gtf -y` (l2r_summary_*), restated in plain Python from the rule as
lr2rmats_amd/csrc/l2r_summaryplan.hip.h states it -- not from its code: the class of a read from its info word, and four
tests/uniq_restatement.merge lists, one per class, each offered its reads in input order.  A read is (tid, info bits, [(start, end),
...]); its strand is the REV bit."""
import numpy as np

from tests import uniq_restatement as ur

KNOWN, KNOWN_SITE, FULL, REV, UNREL = 0x01, 0x02, 0x04, 0x08, 0x10      # L2R_INFO_* (asserted against the header in tests/test_summary_cpu.py)
TID_LIMIT = 1 << 29


def klass(bits):
    if bits & KNOWN:
        return 0
    if bits & KNOWN_SITE:
        return 2 if bits & UNREL else 1
    return 3


def as_transcripts(reads, cls):
    return [(tid, 1 if bits & REV else 0, chain) for tid, bits, chain in reads if klass(bits) == cls]


def per_class(reads, **opts):
    """The four merges: a list of uniq_restatement.merge results."""
    return [ur.merge(as_transcripts(reads, c), **opts) for c in range(4)]


def counts(reads, **opts):
    """The eight numbers of l2r_summary_finish: the reads of every class, then the entries of every class's list."""
    merges = per_class(reads, **opts)
    return [len(m["merged"]) for m in merges] + [len(m["u_src"]) for m in merges]


def in_order(reads):
    """(tid, start) descends inside no class."""
    return all(ur.in_order(as_transcripts(reads, c)) for c in range(4))


def columns(reads):
    """tid, info (the bits and the exon count from bit 8 on), xs, xe."""
    tid = np.asarray([r[0] for r in reads], np.int32)
    info = np.asarray([(r[1] & 0xff) | len(r[2]) << 8 for r in reads], np.uint32)
    xs = np.asarray([e[0] for r in reads for e in r[2]], np.int32)
    xe = np.asarray([e[1] for r in reads for e in r[2]], np.int32)
    return tid, info, xs, xe
