"""Cases of the detail table shared by tests/test_detail_cpu.py and tests/test_gpu_detail.py: a generator of column dicts in the form
tests/detail_restatement.py reads, the case file of tests/detail_dump.hip, and the calls that take a case through capi.Engine."""
import struct

import numpy as np

from lr2rmats_amd import capi
from tests import detail_restatement as dr

EDGES = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000, 999999999, 1000000000, 2147483647]
ALL_FLAGS = 31
ALPHABET = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_.:/-", np.uint8)


def make_case(seed, exons, flags="random", refs=(b"chr1", b"2", b"chrUn_KI270302v1_random"), n_tx=9, name_len=(1, 24), gene_len=(1, 16), no_ref=0.3, coord_max=250000000):
    """A case of len(exons) reads with exons[i] exons each.  flags: "random", or one byte for every exon."""
    rng = np.random.default_rng(seed)
    exons = np.asarray(exons, np.int64)
    n = len(exons)
    ex_off = np.zeros(n + 1, np.int64)
    ex_off[1:] = np.cumsum(exons)
    X = int(ex_off[-1])
    xs, xe = np.zeros(X, np.int32), np.zeros(X, np.int32)
    for i in range(n):
        k = int(exons[i])
        if k:
            steps = rng.integers(1, max(2, coord_max // (2 * k + 1)), 2 * k).astype(np.int64)
            steps[0] = rng.choice([1, 7, 95, 99990, steps[0]])
            c = np.cumsum(steps)
            xs[ex_off[i]:ex_off[i + 1]] = c[0::2]
            xe[ex_off[i]:ex_off[i + 1]] = c[1::2]
    if isinstance(flags, str):
        # sparse, dense and empty reads: a read's density is drawn first
        dens = rng.choice([0.0, 0.05, 0.5, 1.0], n)
        f = (rng.random((X, 5)) < np.repeat(dens, exons)[:, None]).astype(np.uint8) @ np.asarray([1, 2, 4, 8, 16], np.uint8)
        f = f.astype(np.uint8)
    else:
        f = np.full(X, flags, np.uint8)

    def name(lens):
        return bytes(rng.choice(ALPHABET, int(rng.integers(lens[0], lens[1] + 1))))
    names, qname = dr.pack_table([name(name_len) for _ in range(n)])
    anno, ids = dr.pack_table([name(gene_len) for _ in range(2 * n_tx)])
    ref_tx = rng.integers(0, max(n_tx, 1), n).astype(np.int32)
    ref_tx[rng.random(n) < no_ref] = -1
    if n_tx == 0:
        ref_tx[:] = -1
    info = (rng.choice([0, 1, 2, 3, 8, 9, 10, 11, 0xf4, 0xff], n).astype(np.uint32)) | (exons.astype(np.uint32) << 8)
    return {"refs": [bytes(r) for r in refs], "tid": rng.integers(0, len(refs), n).astype(np.int32), "names": names, "qname": np.asarray(qname, np.uint32),
            "anno": anno, "tx_gid": np.asarray(ids[:n_tx], np.uint32), "tx_gname": np.asarray(ids[n_tx:], np.uint32), "ex_off": ex_off, "xs": xs, "xe": xe, "f": f,
            "info": info, "ref_tx": ref_tx}


def case_file(case, first=0, max_rows=1 << 20, max_bytes=1 << 30, fake=(), res_n=-1, res_x=-1, sums_only=0):
    """The case file tests/detail_dump.hip reads."""
    n, refs = len(case["tid"]), case["refs"]
    ref_off = np.zeros(len(refs) + 1, np.int64)
    ref_off[1:] = np.cumsum([len(r) for r in refs])
    head = struct.pack("<13q", n, len(case["xs"]), len(case["names"]), len(refs), len(case["tx_gid"]), len(case["anno"]), first, max_rows, max_bytes, len(fake), res_n, res_x, sums_only)
    body = [np.asarray(case["tid"], np.int32), np.asarray(case["qname"], np.uint32), np.frombuffer(case["names"], np.uint8), np.asarray(case["ex_off"], np.int64),
            np.asarray(case["info"], np.uint32), np.asarray(case["ref_tx"], np.int32), np.asarray(case["xs"], np.int32), np.asarray(case["xe"], np.int32),
            np.asarray(case["f"], np.uint8), ref_off, np.frombuffer(b"".join(refs), np.uint8), np.frombuffer(case["anno"], np.uint8),
            np.asarray(case["tx_gid"], np.uint32), np.asarray(case["tx_gname"], np.uint32), np.asarray(fake, np.uint32)]
    return head + b"".join(a.tobytes() for a in body)


def result_of(case):
    return capi.Result(np.asarray(case["ex_off"], np.int64), np.asarray(case["xs"], np.int32), np.asarray(case["xe"], np.int32), np.asarray(case["f"], np.uint8),
                       np.asarray(case["info"], np.uint32), np.asarray(case["ref_tx"], np.int32))


def engine_rows(eng, case):
    """begin and rows with the case's results uploaded: the bytes of the text."""
    eng.detail_begin(case["refs"], case["anno"], case["tx_gid"], case["tx_gname"])
    return eng.detail_rows(case["tid"], case["names"], case["qname"], result_of(case))


def engine_text(eng, case, max_rows=1 << 20, max_bytes=1 << 30):
    """begin, rows and every batch: (text, n_bytes, the stats after the last batch)."""
    n_bytes = engine_rows(eng, case)
    text = eng.detail_all(len(case["tid"]), max_rows, max_bytes)
    return text, n_bytes, eng.detail_stats()
