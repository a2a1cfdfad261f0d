"""The saturated liberty count of job_liberties (gymgo_amd/csrc/gg_v5.h), restated in numpy: the specification of its formula.

The kernel holds the liberties of a group as R rows of R bits and needs min(number of set bits, 2).  It keeps o = the OR of the
rows and S = their integer sum (R * 2^R < 2^32: nothing is lost), in the kernel's order - row 0 on chain 0 for an odd R, then the
rows in pairs, pair p on chain p % 3, the three chains joined at the end - and returns

    (o != 0) + (((o & -o) ^ S) != 0)

S - o is the sum over the columns c of (n_c - [n_c > 0]) 2^c with n_c = the rows that have column c set, so S == o iff no column
is set in two rows, and S >= o >= the lowest bit of o: S differs from that bit iff a column is set twice or o has two bits.
The longer spelling of the same test, (S != o) or (o & (o - 1)) != 0, is checked next to it.

Cases, at 19, 13 and 9 rows: every single point, every pair of points (the same column in two rows, adjacent columns of one row
and the last column among them), 20 000 random sets of 3 to 40 points, the empty set and the full board.
"""
import itertools

import numpy as np
import pytest


def sat_liberties(rows):
    """rows: uint32 [n, R], one liberty row per board row -> (the kernel's result, the longer spelling's) per set"""
    n, R = rows.shape
    assert R * (1 << R) < 1 << 32
    o3 = np.zeros((3, n), np.uint32)
    s3 = np.zeros((3, n), np.uint32)
    if R & 1:
        o3[0] = rows[:, 0]
        s3[0] = rows[:, 0]
    for r in range(R & 1, R, 2):
        c = (r // 2) % 3
        o3[c] = rows[:, r] | rows[:, r + 1] | o3[c]
        s3[c] = rows[:, r] + rows[:, r + 1] + s3[c]
    o = o3[0] | o3[1] | o3[2]
    s = s3[0] + s3[1] + s3[2]
    low = o & (np.uint32(0) - o)
    kernel = (o != 0).astype(np.int64) + ((low ^ s) != 0)
    longer = (o != 0).astype(np.int64) + ((s != o) | ((o & (o - np.uint32(1))) != 0))
    return kernel, longer


def rows_of(points, R):
    """points: int [n, k] flat point indices (-1: none) -> uint32 [n, R]"""
    n, k = points.shape
    rows = np.zeros((n, R), np.uint32)
    idx = np.arange(n)
    for j in range(k):
        p = points[:, j]
        ok = p >= 0
        np.bitwise_or.at(rows, (idx[ok], p[ok] // R), np.uint32(1) << (p[ok] % R).astype(np.uint32))
    return rows


def popcount(rows):
    return np.unpackbits(rows.view(np.uint8), axis=1).sum(axis=1, dtype=np.int64)


def check(rows, what):
    want = np.minimum(popcount(rows), 2)
    kernel, longer = sat_liberties(rows)
    bad = np.flatnonzero(kernel != want)
    assert len(bad) == 0, (what, len(bad), rows[bad[0]].tolist(), int(kernel[bad[0]]), int(want[bad[0]]))
    assert np.array_equal(longer, want), what


@pytest.mark.parametrize('R', [19, 13, 9])
def test_single_points_pairs_empty_and_full(R):
    P = R * R
    singles = np.arange(P).reshape(P, 1)
    check(rows_of(singles, R), 'single')
    assert (np.minimum(popcount(rows_of(singles, R)), 2) == 1).all()
    pairs = np.array(list(itertools.combinations(range(P), 2)))
    assert len(pairs) == P * (P - 1) // 2 and (R != 19 or len(pairs) == 64980)
    a, b = pairs[:, 0], pairs[:, 1]
    assert ((a % R == b % R)).any() and ((a // R == b // R) & (b == a + 1)).any() and ((a % R == R - 1) & (b % R == R - 1)).any()
    rows = rows_of(pairs, R)
    assert (popcount(rows) == 2).all()
    check(rows, 'pair')
    check(np.zeros((1, R), np.uint32), 'empty')
    check(np.full((1, R), (1 << R) - 1, np.uint32), 'full')


@pytest.mark.parametrize('R', [19, 13, 9])
def test_random_sets_of_3_to_40_points(R):
    rng = np.random.default_rng(1700 + R)
    n, P = 20000, R * R
    k = rng.integers(3, 41, n)
    order = np.argsort(rng.random((n, P)), axis=1)[:, :40]          # forty distinct points per set, the first k of them kept
    pts = np.where(np.arange(40)[None, :] < k[:, None], order, -1)
    rows = rows_of(pts, R)
    assert np.array_equal(popcount(rows), k)
    check(rows, 'random')


def test_three_liberties_whose_sum_is_one_bit():
    """columns c, c, c + 1: S = 2^(c + 2) is a single bit, and o = 2^c | 2^(c + 1) has two"""
    R = 19
    for c in range(R - 1):
        rows = np.zeros((1, R), np.uint32)
        rows[0, 3] = 1 << c
        rows[0, 11] = (1 << c) | (1 << (c + 1))
        s = int(rows.sum())
        assert s & (s - 1) == 0
        check(rows, ('c c c+1', c))
