"""`lr2rmats sort`, `filter -S` and l2r_sort_order on the GPU.  The expected order everywhere is numpy's stable argsort of keys this
file builds from the formula of include/lr2rmats_hip.h:
    key = (tid < 0 ? 0x7fffffff : tid) << 33 | (uint32)(pos + 1) << 1 | (flag >> 4 & 1)"""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

from lr2rmats_amd import capi, hostlib, synth
from oracle import filter_oracle as fo
from tests.test_filter import HDR, _inflate, make_sam

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile():
    text = open(os.path.join(ROOT, "include", "lr2rmats_hip.h")).read()
    return int(re.search(r"#define\s+L2R_SORT_TILE\s+(\d+)", text).group(1))


T = _tile()
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17]


def keys_of(flag, tid, pos):
    t = np.asarray(tid, np.int64)
    t = np.where(t < 0, 0x7fffffff, t).astype(np.uint64)
    p = ((np.asarray(pos, np.int64) + 1) & 0xffffffff).astype(np.uint64)
    s = ((np.asarray(flag, np.int64) >> 4) & 1).astype(np.uint64)
    return (t << np.uint64(33)) | (p << np.uint64(1)) | s


def records_of(key, rng):
    """(flag, tid, pos) whose key is `key` (no key may carry tid 0x7fffffff); the flag bits beside 0x10 are random."""
    key = np.asarray(key, np.uint64)
    tid = (key >> np.uint64(33)).astype(np.int64)
    assert (tid != 0x7fffffff).all()
    pos = (((key >> np.uint64(1)) & np.uint64(0xffffffff)).astype(np.int64) - 1).astype(np.int32)      # (wraps: 0 -> -1, 2^31 -> INT_MIN + ...)
    flag = ((key & np.uint64(1)) << np.uint64(4)).astype(np.uint16) | (rng.integers(0, 0x1000, key.size).astype(np.uint16) & np.uint16(0xfef))
    return flag, tid.astype(np.int32), pos


def expected_passes(key):
    if key.size < 2 or not (key[1:] < key[:-1]).any():
        return 0
    return sum(1 for b in range(8) if np.unique((key >> np.uint64(8 * b)) & np.uint64(0xff)).size > 1)


def check(eng, flag, tid, pos, force=False):
    key = keys_of(flag, tid, pos)
    want = np.argsort(key, kind="stable").astype(np.uint32)
    got = eng.sort_order(flag, tid, pos)
    st = eng.sort_stats()
    assert got.dtype == np.uint32 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    assert st["rows"] == key.size
    in_order = key.size < 2 or not (key[1:] < key[:-1]).any()
    assert st["in_order"] == (1 if in_order else 0)
    assert st["radix_passes"] == ((8 if key.size else 0) if force else expected_passes(key))
    return st


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(0)
    yield e
    e.close()


def _random(n, rng):
    flag = rng.choice(np.array([0, 16, 4, 20, 256, 272, 2048 + 16], np.uint16), n)
    return flag, rng.integers(0, 25, n).astype(np.int32), rng.integers(0, 1 << 28, n).astype(np.int32)


def _heavy_digit(n, rng):
    """One digit value shared by most rows -- far more than 256 in a tile -- in the lowest byte and in the tid byte."""
    heavy = rng.random(n) < 0.8
    pos = np.where(heavy, (rng.integers(0, 1 << 20, n) << 7) | 0x21, rng.integers(0, 1 << 27, n)).astype(np.int32) - 1
    flag = np.where(heavy, 0, rng.choice(np.array([0, 16], np.uint16), n)).astype(np.uint16)
    tid = np.where(rng.random(n) < 0.8, 3, rng.integers(0, 25, n)).astype(np.int32)
    return flag, tid, pos


@pytest.mark.parametrize("n", SIZES)
def test_sort_order_equals_numpy(eng, n, monkeypatch):
    rng = np.random.default_rng(1000 + n)
    # random keys, tid < 25
    flag, tid, pos = _random(n, rng)
    check(eng, flag, tid, pos)
    # all keys equal: the identity
    st = check(eng, np.full(n, 16, np.uint16), np.full(n, 7, np.int32), np.full(n, 12345, np.int32))
    assert st["radix_passes"] == 0
    np.testing.assert_array_equal(eng.sort_order(np.full(n, 16, np.uint16), np.full(n, 7, np.int32), np.full(n, 12345, np.int32)), np.arange(n, dtype=np.uint32))
    # one digit value shared by more than 256 rows of a tile: ranks across waves and rounds
    check(eng, *_heavy_digit(n, rng))
    # reverse-sorted keys (with ties, which must keep their order)
    key = np.sort(keys_of(*_random(n, rng)))[::-1].copy()
    if n:
        key[rng.integers(0, n, n // 8)] = key[0]
        key = np.sort(key)[::-1].copy()
    check(eng, *records_of(key, rng))
    # already sorted: no pass; and the same keys with every pass forced
    rec = records_of(key[::-1].copy(), rng)
    st = check(eng, *rec)
    assert st["radix_passes"] == 0 and st["in_order"] == 1
    monkeypatch.setenv("L2R_SORT_FORCE", "1")
    st = check(eng, *rec, force=True)
    assert st["radix_passes"] == (8 if n else 0)
    check(eng, flag, tid, pos, force=True)
    monkeypatch.delenv("L2R_SORT_FORCE")
    # tid in {-1, 0, 0x7ffffffe} x pos in {-1, 0, 2^31 - 2} x both strands
    tid = rng.choice(np.array([-1, 0, 0x7ffffffe], np.int32), n)
    pos = rng.choice(np.array([-1, 0, 2 ** 31 - 2], np.int32), n)
    check(eng, rng.choice(np.array([0, 16, 4, 20], np.uint16), n), tid, pos)
    # the strand bit as the only difference
    check(eng, rng.choice(np.array([0, 16, 0xfef, 0xfff], np.uint16), n), np.full(n, 2, np.int32), np.full(n, 99, np.int32))


@pytest.mark.parametrize("byte", range(8))
def test_keys_that_differ_in_one_byte_take_one_pass(eng, byte):
    rng = np.random.default_rng(50 + byte)
    base = np.uint64(0x0305_0709_0b0d_0f10)
    for n in (65, 257, T + 1, 3 * T + 17):
        v = rng.integers(0, 0x80 if byte == 7 else 0x100, n).astype(np.uint64)
        key = (base & ~(np.uint64(0xff) << np.uint64(8 * byte))) | (v << np.uint64(8 * byte))
        flag, tid, pos = records_of(key, rng)
        np.testing.assert_array_equal(keys_of(flag, tid, pos), key)
        st = check(eng, flag, tid, pos)
        assert st["radix_passes"] == 1


def test_a_million_rows(eng):
    rng = np.random.default_rng(7)
    n = 1 << 20
    flag, tid, pos = _random(n, rng)
    pos[rng.integers(0, n, n // 4)] = 4242                       # ties
    st = check(eng, flag, tid, pos)
    assert st["radix_passes"] == 5                              # strand + 28 bits of position: bytes 0..3; tid < 25: byte 4


def test_two_calls_on_one_context_larger_then_smaller():
    e = capi.Engine(0)
    try:
        rng = np.random.default_rng(9)
        check(e, *_random(5 * T + 3, rng))
        check(e, *_random(T + 9, rng))
        check(e, *_heavy_digit(300, rng))
        check(e, *_random(2 * T, rng))
    finally:
        e.close()


def test_the_row_limit_fails_before_any_pointer_is_read(eng):
    lib = capi.load_library()
    limit = 2 ** 32 - 1 - T
    recs = capi.CSortRecords(limit + 1, None, None, None)
    rc = lib.l2r_sort_order(eng.ctx, C.byref(recs), None)
    msg = lib.l2r_last_error().decode()
    assert rc != 0 and "l2r_sort_order" in msg and str(limit + 1) in msg
    st = eng.sort_stats()
    assert st["rows"] == 0 and st["radix_passes"] == 0
    recs = capi.CSortRecords(-1, None, None, None)
    assert lib.l2r_sort_order(eng.ctx, C.byref(recs), None) != 0
    recs = capi.CSortRecords(0, None, None, None)
    assert lib.l2r_sort_order(eng.ctx, C.byref(recs), None) == 0
    check(eng, *_random(100, np.random.default_rng(3)))          # the context is as good as before


# ---------------------------------------------------------------------------------------------------- the commands

def _record_keys(recs, idx):
    flag = np.array([r.flag for r in recs], np.int64)
    tid = np.array([-1 if r.rname == "*" else idx[r.rname] for r in recs], np.int64)
    pos = np.array([r.pos - 1 for r in recs], np.int64)
    return keys_of(flag, tid, pos)


def _expected_sorted_stream(sam, keep=None):
    header, refs, recs = fo.parse_sam(sam)
    idx = {name: i for i, (name, _) in enumerate(refs)}
    if keep is not None:
        recs = [recs[i] for i in keep]
    order = np.argsort(_record_keys(recs, idx), kind="stable") if recs else []
    header = [l.replace("SO:unsorted", "SO:coordinate") for l in header]
    assert any("SO:coordinate" in l for l in header)
    return fo.header_bytes(header, refs) + b"".join(fo.encode_record(recs[int(i)], idx) for i in order), len(recs)


def _shuffled_sam(path, n_reads, seed):
    """make_sam's records (unmapped ones among them) in random order, every fifth mapped one moved to one of three places so that
    many keys tie."""
    tmp = path + ".tmp"
    make_sam(tmp, n_reads, seed)
    rng = np.random.default_rng(seed)
    head = [l for l in open(tmp) if l.startswith("@")]
    body = [l for l in open(tmp) if not l.startswith("@")]
    for k in range(0, len(body), 5):
        f = body[k].split("\t")
        if f[2] != "*":
            f[2], f[3] = "chr2", str(int(rng.choice([777, 778, 40000])))
            body[k] = "\t".join(f)
    rng.shuffle(body)
    with open(path, "w") as fh:
        fh.writelines(head + body)
    os.remove(tmp)
    return len(body)


def _cli(args, stdout_path=None, rc=0):
    r = hostlib.run_cli(args, stdout_path=stdout_path)
    assert r.returncode == rc, r.stderr.decode()[-2000:]
    return r


def test_sort_command_sam_bam_and_gzip_input(tmp_path):
    sam, out = str(tmp_path / "in.sam"), str(tmp_path / "out.bam")
    n = _shuffled_sam(sam, 1500, 31)
    want, n_rec = _expected_sorted_stream(sam)
    assert n_rec == n > 2500 and sum(1 for l in open(sam) if l.split("\t")[2:3] == ["*"]) > 10
    r = _cli(["sort", sam], stdout_path=out)
    assert ("[bam_sort] Sorted alignments: %d\n" % n) in r.stderr.decode()
    got = _inflate(out)                                          # (asserts the BGZF end-of-file block)
    assert got == want
    assert b"@HD\tVN:1.6\tSO:coordinate\n" in got[:200]
    assert _cli(["sort-check", out]).stdout.startswith(b"coordinate sorted")
    assert b"not coordinate sorted" in _cli(["sort-check", sam], rc=1).stdout
    # -o, and the same records as a BAM file and as gzip-compressed SAM
    header, refs, recs = fo.parse_sam(sam)
    idx = {name: i for i, (name, _) in enumerate(refs)}
    bam, samgz, out2 = str(tmp_path / "in.bam"), str(tmp_path / "in.sam.gz"), str(tmp_path / "out2.bam")
    open(bam, "wb").write(fo.bgzf_blocks(fo.header_bytes(header, refs) + b"".join(fo.encode_record(r, idx) for r in recs)))
    with open(sam, "rb") as fi, gzip.open(samgz, "wb", compresslevel=1) as fz:
        fz.write(fi.read())
    for src in (bam, samgz):
        r = _cli(["sort", "-o", out2, src])
        assert r.stdout == b"" and _inflate(out2) == want, src
    # sorting what is sorted already changes nothing
    _cli(["sort", "--output", out2, out])
    assert _inflate(out2) == want


def test_sort_command_empty_and_header_only_inputs(tmp_path):
    out = str(tmp_path / "out.bam")
    hdr_only = str(tmp_path / "h.sam")
    open(hdr_only, "w").write(HDR)
    _cli(["sort", hdr_only], stdout_path=out)
    assert _inflate(out) == _expected_sorted_stream(hdr_only)[0]
    empty = str(tmp_path / "e.sam")
    open(empty, "w").write("")
    _cli(["sort", empty], stdout_path=out)
    assert _inflate(out) == fo.header_bytes(["@HD\tVN:1.6\tSO:coordinate\n"], [])
    assert _cli(["sort-check", out]).stdout.startswith(b"coordinate sorted: 0 records")


def test_filter_sorted_is_filter_then_the_order(tmp_path):
    sam, out = str(tmp_path / "in.sam"), str(tmp_path / "out.bam")
    n = make_sam(sam, 3000, 11)
    plain, keep = fo.expected_stream(sam)
    assert 300 < len(keep) < n
    _cli(["filter", sam], stdout_path=out)
    assert _inflate(out) == plain                                # plain filter: what the oracle route says, as before
    want, n_rec = _expected_sorted_stream(sam, keep)
    assert n_rec == len(keep) and want != plain
    for flag_arg in ("-S", "--sorted"):
        r = _cli(["filter", flag_arg, sam], stdout_path=out)
        assert _inflate(out) == want
        assert ("[bam_filter] Filtered alignments: %d\n" % len(keep)) in r.stderr.decode()
    assert _cli(["sort-check", out]).returncode == 0
    # with other options in front and behind
    kw = dict(cov_rate=0.8, map_qual=0.9, sec_rat=0.95)
    keep2 = fo.expected_stream(sam, **kw)[1]
    _cli(["filter", "-v", "0.8", "-S", "-q", "0.9", "-s", "0.95", sam], stdout_path=out)
    assert _inflate(out) == _expected_sorted_stream(sam, keep2)[0]


def test_sort_feeds_update_gtf(tmp_path):
    """`sort` of a shuffled alignment file, then update-gtf -l 3 -A -E == update-gtf on a SAM this test ordered with numpy."""
    anno = synth.make_annotation(6000, 77, nchr=4)
    reads = synth.make_reads(anno, 4000, 5, 77)
    sam, gtf = str(tmp_path / "r.sam"), str(tmp_path / "anno.gtf")
    reads.write_sam(sam)
    anno.write_gtf(gtf)
    head = [l for l in open(sam) if l.startswith("@")]
    body = [l for l in open(sam) if not l.startswith("@")]
    names = [l.split("\t")[1][3:] for l in head if l.startswith("@SQ")]
    rng = np.random.default_rng(5)
    rng.shuffle(body)
    shuf, mine, sbam = str(tmp_path / "shuf.sam"), str(tmp_path / "mine.sam"), str(tmp_path / "sorted.bam")
    open(shuf, "w").writelines(head + body)
    f = [l.split("\t") for l in body]
    key = keys_of([int(x[1]) for x in f], [names.index(x[2]) for x in f], [int(x[3]) - 1 for x in f])
    assert (key[1:] < key[:-1]).any()
    open(mine, "w").writelines(head + [body[int(i)] for i in np.argsort(key, kind="stable")])
    assert _cli(["sort-check", shuf], rc=1) and _cli(["sort-check", mine])
    _cli(["sort", "-o", sbam, shuf])
    outs = {}
    for tag, src in (("a", sbam), ("b", mine)):
        o = [str(tmp_path / ("out_%s.%s" % (tag, x))) for x in ("gtf", "detail", "bed")]
        _cli(["update-gtf", "-l", "3", "-A", o[1], "-E", o[2], src, gtf], stdout_path=o[0])
        outs[tag] = [open(p, "rb").read() for p in o]
    assert all(len(x) > 100 for x in outs["a"])
    assert outs["a"] == outs["b"]
