"""Records for the tests of `bam2bed` (tests/test_bed12_cpu.py, tests/test_gpu_bed12.py): the edges of the rule and of the kernels, as
lists of (flag, tid, pos, mapq, name, cigar) -- the records of tests/bed12_restatement.py."""
import numpy as np

from tests import bed12_restatement as br

REFS = [b"chr1", b"chr2", b"chrM", b"chrUn_KI270302v1", b"c"]
M, I, D, N, S, H, P, EQ, X = range(9)
OP_MAX = (1 << 28) - 1                                              # the longest operation a CIGAR word holds
DIGIT_EDGES = [0, 9, 10, 99999, 100000, 999999999, 1000000000]


def rec(flag=0, tid=0, pos=0, mapq=60, name=b"r", cigar=((10, M),)):
    return (flag, tid, pos, mapq, name, list(cigar))


def long_op(v, op=M):
    """v reference bases as operations of one kind (a word holds 28 bits of length)."""
    out = []
    while v > OP_MAX:
        out.append((OP_MAX, op))
        v -= OP_MAX
    return out + [(v, op)]


def ops_record(k, seed=0, **kw):
    """A record of exactly k operations of every kind, about a third of them N."""
    rng = np.random.default_rng(1000 + 7 * k + seed)
    ops = rng.choice([M, I, D, N, S, H, P, EQ, X, N, N, M], size=k)
    return rec(cigar=[(int(rng.integers(0, 3000)), int(op)) for op in ops], name=b"ops%d_%d" % (k, seed), **kw)


def blocks_record(b, seed=0, **kw):
    """A record of exactly b blocks."""
    rng = np.random.default_rng(2000 + 11 * b + seed)
    cig = []
    for j in range(b):
        if j:
            cig.append((int(rng.integers(1, 5000)), N))
        cig.append((int(rng.integers(1, 300)), M))
    return rec(cigar=cig, name=b"blk%d_%d" % (b, seed), **kw)


def random_records(rng, n, max_ops=12, unmapped=0.1):
    out = []
    for i in range(n):
        flag = int(rng.choice([0, 16, 64, 128, 192, 80, 144, 256, 2048 + 16]))
        if rng.random() < unmapped:
            flag |= 4
        k = int(rng.integers(0, max_ops + 1))
        ops = rng.choice([M, I, D, N, S, H, P, EQ, X, M, M, N], size=k)
        cig = [(int(rng.integers(0, 2000)), int(op)) for op in ops]
        name = bytes(rng.integers(65, 123, size=int(rng.integers(1, 41))).astype(np.uint8))          # 'A' .. 'z'
        out.append((flag, int(rng.integers(0, len(REFS))), int(rng.integers(0, 200000000)), int(rng.integers(0, 256)), name, cig))
    return out


def digit_edge_records():
    """pos, a block size and a block start at every digit edge."""
    out = []
    for v in DIGIT_EDGES:
        out.append(rec(pos=v, name=b"pos%d" % v))
        out.append(rec(cigar=long_op(v) + [(7, N), (3, M)], name=b"size%d" % v))                   # sizes v,3
        out.append(rec(cigar=[(1, M)] + long_op(v - 1, N) + [(1, M)] if v else [(0, N), (1, M)], name=b"start%d" % v))      # starts 0,v
    return out


def end_limit_records(over):
    """Three records, the second of which ends at 2147483647 (over = 0) or one beyond."""
    return [rec(name=b"before"), rec(pos=br.POS_MAX - 100, cigar=[(60, M), (30, N), (10 + over, M)], name=b"limit"), rec(name=b"behind")]


def residue_records():
    """Name lengths 1..16 twice over: the line offsets take every residue modulo 16."""
    return [rec(name=b"n" * (1 + k % 16), pos=5) for k in range(40)]


def flag_records():
    return [rec(flag=f, name=b"f%d" % f, cigar=[(4, M), (6, N), (5, M)]) for f in (0, 16, 64, 128, 192, 80, 144, 208, 1, 2048)]


def unmapped_records(tile):
    """Unmapped records first, last, and a whole tile of them (with every tid, and a CIGAR nobody looks at)."""
    u = lambda k: (4 | (16 if k % 2 else 0), -1 if k % 3 else 99, -1, 0, b"u%d" % k, [(5, 12)] if k % 5 == 0 else [])
    return [u(0)] + [rec(name=b"a%d" % k) for k in range(tile - 1)] + [u(k) for k in range(1, tile + 1)] + [rec(name=b"b", pos=77), u(7)]


def tile_text_records(tile, target, ref_names=REFS):
    """`tile` records in front (short lines whose bytes are no multiple of 16, so that the tile behind starts off a 16-byte boundary)
    and `tile` records whose lines are exactly `target` bytes together, set by their name lengths."""
    front = [rec(name=b"f", pos=k % 7) for k in range(tile)]
    if len(br.text(front, ref_names)) % 16 == 0:
        front[0] = rec(name=b"ff", pos=0)
    base = len(br.line(rec(name=b""), ref_names))
    need = target - tile * (base + 1)
    assert 0 <= need <= tile * 253, "target out of reach"
    lens = [1 + min(253, max(0, need - 253 * k)) for k in range(tile)]
    back = [rec(name=b"x" * n) for n in lens]
    assert len(br.text(back, ref_names)) == target
    return front + back


def bound_worst_records():
    """Records built to be worst for bed_line_bound: every number at ten digits, the longest name, every operation an N."""
    big = 1000000000
    ten = rec(pos=big, mapq=255, name=b"q" * 254, flag=192, tid=3, cigar=[(1, M)] + long_op(big - 1, N) + [(1, M)])      # start, end, a block start at ten digits
    all_n = rec(pos=big, mapq=100, name=b"z" * 254, tid=3, cigar=long_op(big, N) + [(1, N)] * 40)                            # every operation an N
    sizes = rec(pos=1, name=b"s", cigar=long_op(big, M) + [(1, N)] + long_op(big, D))                                        # block sizes at ten digits
    return [ten, all_n, sizes, rec(cigar=[]), rec(cigar=[(0, N)] * 65)]
