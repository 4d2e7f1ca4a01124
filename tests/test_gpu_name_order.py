"""`lr2rmats sort -n`, `filter -N`, `fusion -N` and l2r_name_order on the GPU.  The expected order everywhere is that of
tests/name_order_restatement.py: a dict of first appearance, then a stable sort by (first, index)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lr2rmats_amd import capi, hostlib
from tests import name_order_restatement as nr
from tests import test_fusion as tf
from tests.test_filter import _inflate, make_sam

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile():
    text = open(os.path.join(ROOT, "include", "lr2rmats_hip.h")).read()
    return int(re.search(r"#define\s+L2R_SORT_TILE\s+(\d+)", text).group(1))


T = _tile()
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17]


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(0)
    yield e
    e.close()


def _rand_name(rng, lo=1, hi=254):
    return bytes(rng.integers(1, 256, int(rng.integers(lo, hi + 1))).astype(np.uint8))


def random_names(n, rng):
    """Names of 1..254 bytes with 1..5 records each, shuffled."""
    names = []
    while len(names) < n:
        names += [_rand_name(rng)] * int(rng.integers(1, 6))
    names = names[:n]
    return [names[int(i)] for i in rng.permutation(n)]


def grouped(names):
    return [names[i] for i in nr.name_order(names)[0]]


def one_large_group(n, rng):
    """One name on more than a tile of records (where n has that many), singletons between them."""
    big = min(n, max(T + 5, n // 2 + 1)) if n > T else n // 2 + 1
    names = [b"the/large/group"] * min(big, n) + [b"single%07d" % k for k in range(n - min(big, n))]
    return [names[int(i)] for i in rng.permutation(n)]


def prefix_and_last_byte_pairs(n, rng):
    """Every name is a prefix of the next one of its family, or differs from a sibling in its last byte only."""
    base = [_rand_name(rng, 200, 240) for _ in range(3)] + [b"read", b"r"]
    pool = []
    for b in base:
        pool += [b[:k] for k in (1, 2, 7, 8, 9, 15, 16, 17, len(b) - 1, len(b)) if 0 < k <= len(b)]
        pool += [b + bytes([c]) for c in (1, 2, 0x7f, 0x80, 0xff)] + [b + b"\x01\x01", b + b"\x01\x02"]
    return [pool[int(i)] for i in rng.integers(0, len(pool), n)]


def check(eng, names, route=0):
    want, groups = nr.name_order(names)
    got, n_groups = eng.name_order(names)
    st = eng.name_stats()
    assert got.dtype == np.uint32 and got.shape == (len(names),)
    np.testing.assert_array_equal(got, np.asarray(want, np.uint32))
    assert n_groups == groups
    assert st["rows"] == len(names) and st["groups"] == groups
    assert st["identity"] == (1 if want == list(range(len(names))) else 0)
    if route is not None:
        assert st["route"] == route, st
        if route == 0:
            assert st["mismatches"] == 0
    return st


@pytest.mark.parametrize("n", SIZES)
def test_name_order_equals_the_restatement(eng, n):
    rng = np.random.default_rng(2000 + n)
    names = random_names(n, rng)
    check(eng, names)
    st = check(eng, grouped(names))                               # grouped already: the identity
    assert st["identity"] == 1
    st = check(eng, [b"one/name"] * n)
    assert st["groups"] == min(n, 1) and st["identity"] == 1 and st["radix_passes"] == 0
    st = check(eng, [b"read%08d" % int(k) for k in rng.permutation(n)])
    assert st["groups"] == n and st["identity"] == 1
    check(eng, one_large_group(n, rng))
    check(eng, prefix_and_last_byte_pairs(n, rng))
    check(eng, [b""] * (n // 3) + random_names(n - n // 3, rng))  # the empty name is a name


def test_every_pass_forced(eng, monkeypatch):
    rng = np.random.default_rng(5)
    names = random_names(T + 1, rng)
    free = eng.name_order(names)[0]
    assert 0 < eng.name_stats()["radix_passes"] <= 8
    monkeypatch.setenv("L2R_SORT_FORCE", "1")
    st = check(eng, names)
    assert st["radix_passes"] == 8
    np.testing.assert_array_equal(eng.name_order(names)[0], free)
    st = check(eng, grouped(names))
    assert st["radix_passes"] == 8 and st["identity"] == 1


@pytest.mark.parametrize("bits", [0, 1, 8])
@pytest.mark.parametrize("n", [257, T + 1])
def test_few_hash_bits_take_the_host_route(eng, monkeypatch, n, bits):
    rng = np.random.default_rng(300 + n)
    names = random_names(n, rng)
    monkeypatch.setenv("L2R_NAME_HASH_BITS", str(bits))
    st = check(eng, names, route=2)
    assert st["mismatches"] > 0
    if bits == 0:
        assert st["radix_passes"] == 0
    monkeypatch.setenv("L2R_NAME_HASH_BITS", "64")
    st = check(eng, names, route=0)
    assert st["mismatches"] == 0
    monkeypatch.delenv("L2R_NAME_HASH_BITS")
    check(eng, names, route=0)


def test_two_calls_on_one_context_larger_then_smaller():
    e = capi.Engine(0)
    try:
        rng = np.random.default_rng(9)
        check(e, random_names(5 * T + 3, rng))
        check(e, random_names(T + 9, rng))
        check(e, one_large_group(300, rng))
        # beside a coordinate sort in the same buffers: what l2r_sort_stats says of it stays
        flag, tid, pos = np.zeros(500, np.uint16), rng.integers(0, 5, 500).astype(np.int32), rng.integers(0, 1 << 20, 500).astype(np.int32)
        order = e.sort_order(flag, tid, pos)
        before = e.sort_stats()
        check(e, random_names(2 * T, rng))
        assert e.sort_stats() == before
        np.testing.assert_array_equal(e.sort_order(flag, tid, pos), order)
    finally:
        e.close()


def test_argument_errors_launch_nothing(eng):
    lib = capi.load_library()
    check(eng, [b"a", b"b", b"a"])
    groups = C.c_int64(-1)
    order = np.zeros(4, np.uint32)
    blob = np.frombuffer(b"x" * 600, np.uint8)

    def call(n, off, names, out=order, ran=False):
        off = None if off is None else np.asarray(off, np.int64)
        recs = capi.CNameRecords(n, None if off is None else off.ctypes.data, names)
        rc = lib.l2r_name_order(eng.ctx, C.byref(recs), None if out is None else out.ctypes.data, C.byref(groups))
        st = eng.name_stats()
        assert ran or (st["rows"] == 0 and st["radix_passes"] == 0 and st["groups"] == 0)          # nothing ran
        return rc, lib.l2r_last_error().decode()

    for args in ((3, None, blob.ctypes.data), (3, [0, 1, 2, 3], None), (3, [0, 1, 2, 3], blob.ctypes.data, None)):
        rc, msg = call(*args)
        assert rc != 0 and "l2r_name_order" in msg and "null column" in msg
    rc, msg = call(3, [0, 4, 2, 6], blob.ctypes.data)
    assert rc != 0 and "l2r_name_order" in msg and "descends" in msg and "record 1" in msg
    rc, msg = call(3, [0, 3, 258, 260], blob.ctypes.data)
    assert rc != 0 and "l2r_name_order" in msg and "255" in msg and "record 1" in msg
    limit = 2 ** 32 - 1 - T
    rc, msg = call(limit + 1, None, None, None)
    assert rc != 0 and str(limit + 1) in msg
    assert call(-1, None, None, None)[0] != 0
    rc, _ = call(0, None, None, None)
    assert rc == 0 and groups.value == 0
    rc, _ = call(2, [0, 254, 508], blob.ctypes.data, ran=True)              # 254 bytes is a name; the context is as good as before
    assert rc == 0 and groups.value == 1 and order[:2].tolist() == [0, 1]
    check(eng, random_names(100, np.random.default_rng(3)))


# ---------------------------------------------------------------------------------------------------- the commands

def _cli(args, stdout_path=None, rc=0):
    r = hostlib.run_cli(args, stdout_path=stdout_path)
    assert r.returncode == rc, r.stderr.decode()[-2000:]
    return r


def _records(bam):
    """(header text, [record bytes]) of a BAM file."""
    raw = _inflate(bam)
    l_text = int.from_bytes(raw[4:8], "little")
    text = raw[8:8 + l_text]
    at = 8 + l_text
    n_ref = int.from_bytes(raw[at:at + 4], "little"); at += 4
    for _ in range(n_ref):
        at += 4 + int.from_bytes(raw[at:at + 4], "little") + 4
    recs = []
    while at < len(raw):
        size = int.from_bytes(raw[at:at + 4], "little")
        recs.append(raw[at:at + 4 + size]); at += 4 + size
    return text, recs


def _name(rec):
    return rec[36:36 + rec[12] - 1]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """A small SAM of multi-alignment reads (tests/test_filter.py's make_sam), its coordinate form and the `sort -n` form of that."""
    d = tmp_path_factory.mktemp("name_order")
    f = {k: str(d / v) for k, v in dict(sam="in.sam", coord="coord.bam", named="named.bam").items()}
    f["n"] = make_sam(f["sam"], 150, 23)
    _cli(["sort", "-o", f["coord"], f["sam"]])
    r = _cli(["sort", "-n", "-o", f["named"], f["coord"]])
    f["stderr"] = r.stderr.decode()
    return f


def test_sort_n_of_the_coordinate_form(files):
    assert 250 < files["n"] < 600
    text_c, coord = _records(files["coord"])
    text_n, named = _records(files["named"])
    assert b"SO:coordinate" in text_c and _cli(["sort-check", files["coord"]]).returncode == 0
    names_c = [_name(r) for r in coord]
    bad = nr.is_grouped(names_c)
    assert bad is not None                                          # the coordinate form spreads a read's alignments
    out = _cli(["sort-check", "-n", files["coord"]], rc=1).stdout.decode()
    assert ('record %d ("%s")' % (bad, names_c[bad].decode())) in out
    # the name form: grouped, the same records, in the restatement's order, and the header says so
    assert _cli(["sort-check", "-n", files["named"]]).stdout.startswith(b"name grouped: %d records" % len(coord))
    assert sorted(named) == sorted(coord) and len(named) == files["n"]
    order, groups = nr.name_order(names_c)
    assert named == [coord[i] for i in order]
    assert ("[bam_sort] Grouped alignments: %d in %d reads\n" % (len(coord), groups)) in files["stderr"]
    hd = text_n.split(b"\n")[0].split(b"\t")
    assert hd[0] == b"@HD" and b"SO:unsorted" in hd and b"GO:query" in hd and b"SO:coordinate" not in text_n
    assert text_n.split(b"\n")[1:] == text_c.split(b"\n")[1:]


def test_sort_n_of_a_grouped_file_keeps_its_order(files, tmp_path):
    again = str(tmp_path / "again.bam")
    _cli(["sort", "--name", files["named"]], stdout_path=again)
    assert _inflate(again) == _inflate(files["named"])
    # and plain `sort` of the name form is the coordinate form again, byte for byte what `sort` gave before
    back = str(tmp_path / "back.bam")
    _cli(["sort", "-o", back, files["named"]])
    text_b, recs_b = _records(back)
    assert b"SO:coordinate" in text_b and _cli(["sort-check", back]).returncode == 0 and sorted(recs_b) == sorted(_records(files["coord"])[1])


def test_filter_N_is_filter_behind_sort_n(files, tmp_path):
    out = {k: str(tmp_path / (k + ".bam")) for k in ("coord_plain", "coord_N", "named_plain", "named_N", "NS", "S")}
    _cli(["filter", files["named"]], stdout_path=out["named_plain"])
    r = _cli(["filter", "-N", files["coord"]], stdout_path=out["coord_N"])
    want = _inflate(out["named_plain"])
    assert _inflate(out["coord_N"]) == want
    n_kept = len(_records(out["named_plain"])[1])
    assert n_kept > 30 and ("[bam_filter] Filtered alignments: %d\n" % n_kept) in r.stderr.decode()
    # without -N every fragment of a read is judged as a read of its own: the defect the option removes
    _cli(["filter", files["coord"]], stdout_path=out["coord_plain"])
    assert sorted(_records(out["coord_plain"])[1]) != sorted(_records(out["named_plain"])[1])
    # on name-grouped input -N changes nothing
    _cli(["filter", "--group-names", files["named"]], stdout_path=out["named_N"])
    assert _inflate(out["named_N"]) == want
    # -N -S: group, select, then the coordinate order
    _cli(["filter", "-N", "-S", files["coord"]], stdout_path=out["NS"])
    assert _cli(["sort-check", out["NS"]]).returncode == 0
    _cli(["filter", "-S", files["named"]], stdout_path=out["S"])
    text_ns, recs_ns = _records(out["NS"])
    assert b"SO:coordinate" in text_ns and sorted(recs_ns) == sorted(_records(out["named_plain"])[1])
    assert recs_ns == _records(out["S"])[1]


def test_fusion_N_is_fusion_behind_sort_n(tmp_path):
    sam, coord, named = (str(tmp_path / x) for x in ("in.sam", "coord.bam", "named.bam"))
    tf.make_sam(sam, 200, 41)
    _cli(["sort", "-o", coord, sam])
    _cli(["sort", "-n", "-o", named, coord])
    got = {}
    for tag, args in (("named", [named]), ("coord_N", ["-N", coord]), ("coord", [coord]), ("named_N", ["--group-names", named])):
        site = str(tmp_path / (tag + ".site"))
        r = _cli(["fusion", "-f", site] + args)
        got[tag] = (r.stdout, open(site, "rb").read(), re.search(r"transcripts: (\d+)", r.stderr.decode()).group(1))
    assert int(got["named"][2]) > 10
    assert got["coord_N"] == got["named"] and got["named_N"] == got["named"]
    assert got["coord"] != got["named"] and int(got["coord"][2]) < int(got["named"][2])
