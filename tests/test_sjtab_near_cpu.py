"""The second filter stage of `sjtab` without a GPU: the two forms of its restatement against each other and against the hand-worked
table, and the -m list as the command parses it."""
import numpy as np
import pytest

from tests import sjtab_near_restatement as nr
from tests import sjtab_restatement as st


def _both_forms(rows9, filt, dist_min, intron_max):
    left, n_long, n_near = nr.filter2(rows9, filt, dist_min, intron_max)
    got = nr.filter2_numpy(nr.columns(rows9), filt, dist_min, intron_max)
    assert [r for r, k in zip(rows9, got["keep"]) if k] == left
    assert (got["n_long"], got["n_near"]) == (n_long, n_near)
    s1, _ = nr.stage1(rows9, filt, intron_max)
    assert [r for r, k in zip(rows9, got["s1"]) if k] == s1
    _, near = nr.stage2(s1, (1,) * 5)
    assert [d for d, _ in near] == got["dd"].tolist() and [a for _, a in near] == got["da"].tolist()
    return left, n_long, n_near


def test_hand_table():
    assert nr.HAND_ROWS == sorted(nr.HAND_ROWS) and len(set(r[:3] for r in nr.HAND_ROWS)) == len(nr.HAND_ROWS)
    left, n_long, n_near = _both_forms(nr.HAND_ROWS, nr.HAND_FILTER, nr.HAND_DIST, nr.HAND_INTRON_MAX)
    assert left == [r for r, s in zip(nr.HAND_ROWS, nr.HAND_STAYS) if s]
    assert (n_long, n_near) == (nr.HAND_N_LONG, nr.HAND_N_NEAR)
    assert nr.HAND_STAYS.count(False) == n_long + n_near + 1               # ... and the one row of stage 1's old test
    # the distances the reasons quote
    s1, _ = nr.stage1(nr.HAND_ROWS, nr.HAND_FILTER, nr.HAND_INTRON_MAX)
    near = dict(zip([r[:3] for r in s1], nr.stage2(s1, nr.HAND_DIST)[1]))
    assert near[(0, 1000, 1300)] == (0, 200) and near[(0, 3100, 3509)] == (100, 9) and near[(0, 5100, 5510)] == (100, 10)
    assert near[(0, 11012, 11600)][0] == 7 and near[(0, 9000, 9100)][0] > 1000
    assert near[(1, 1000, 1100)] == (nr.FAR, nr.FAR) and near[(2, 1000, 1300)] == (nr.FAR, nr.FAR)
    # both switched off: the table of sjtab_restatement.kept, and with the distances alone no row goes for its length
    assert nr.filter2(nr.HAND_ROWS, nr.HAND_FILTER) == ([r for r in nr.HAND_ROWS if st.kept(r[5], r[4], r[6], r[7], r[8], nr.HAND_FILTER)], 0, 0)
    assert nr.filter2(nr.HAND_ROWS, nr.HAND_FILTER, nr.HAND_DIST)[1:] == (0, nr.HAND_N_NEAR)


@pytest.mark.parametrize("seed", range(6))
def test_forms_agree_on_random_tables(seed):
    rng = np.random.default_rng(seed)
    cols = nr.random_rows(seed, 300, n_tid=3, span=int(rng.choice([200, 2000, 20000])), len_max=int(rng.choice([60, 5000])))
    rows9 = [tuple(int(c[i]) for c in cols) for i in range(len(cols[0]))]
    assert rows9 == sorted(rows9)
    dist = tuple(int(v) for v in rng.integers(0, 12, 5))
    lens = tuple(int(v) for v in rng.integers(20, 5000, int(rng.integers(0, 9))))
    filt = ((0, 20, 5, 5, 5), (0, 2, 1, 1, 1), (0, 3, 1, 1, 1))
    left, n_long, n_near = _both_forms(rows9, filt, dist, lens)
    _both_forms(rows9, st.KEEP_ALL, dist, ())
    _both_forms(rows9, filt, (0,) * 5, lens)
    if seed == 0:
        assert 0 < len(left) < len(rows9) and n_near > 0


def test_extremes_of_the_rule():
    big = 0x7fffffff
    # differences beyond 31 bits clamp; equal coordinates give 0; a motif above 6 is motif 0
    rows = [(0, -big, -big + 5, 0, 0, 0, 9, 0, 50), (0, big - 7, big, 0, 0, 0, 9, 0, 50), (1, 5, 9, 0, 7, 0, 9, 0, 50), (1, 5, 30, 0, 0, 0, 9, 0, 50)]
    _, near = nr.stage2(rows, (1,) * 5)
    assert near == [(nr.FAR, nr.FAR), (nr.FAR, nr.FAR), (0, 21), (0, 21)]
    got = nr.filter2_numpy(nr.columns(rows), st.KEEP_ALL, (0, 1, 0, 0, 0), ())
    assert got["dd"].tolist() == [nr.FAR, nr.FAR, 0, 0] and got["da"].tolist() == [nr.FAR, nr.FAR, 21, 21] and got["keep"].tolist() == [True, True, False, False]
    assert nr.filter2(rows, st.KEEP_ALL, (0, 1, 0, 0, 0))[0] == rows[:2]
    # 64-bit length
    assert nr.too_long((0, -big, big, 0, 0, 0, 1, 0, 50), (big,)) and not nr.too_long((0, 1, big, 0, 0, 0, 1, 0, 50), (big,))


def test_int_list_of_the_command():
    from lr2rmats_amd import hostlib
    if not hasattr(hostlib, "sj_int_list"):
        pytest.fail("hostlib.sj_int_list is missing: sjtab -m is not built")
    assert hostlib.sj_int_list("50000,100000,200000") == [50000, 100000, 200000]
    assert hostlib.sj_int_list("7") == [7]
    assert hostlib.sj_int_list("1,2,3,4,5,6,7,2147483647") == [1, 2, 3, 4, 5, 6, 7, 2147483647]
    assert hostlib.sj_int_list("0") == [0]
    for bad in ("1,2,3,4,5,6,7,8,9", "", "1,", "1,,2", "-1", "1 2", "1,x", ",1", "+1", "2147483648", "1,-2"):
        assert hostlib.sj_int_list(bad) is None, bad
