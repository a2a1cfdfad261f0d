"""CPU: what tests/test_gpu_plane_sizes.py relies on, without a device - at every board size from 2 to 19 the two
generators of tests/plane_cases.py give valid boards, the expectation on them is not vacuous (ended and running games, all
four life and ladder planes, chains without a liberty, ladders deeper than any policy position holds), and the expectation
modules agree with themselves under the eight orientations, even N included: the reference checking the reference."""
import numpy as np
import pytest

import features_expect as fe
import ladder_expect as lad
import life_expect as life
import plane_cases as pc
import symmetry_expect as se
import test_gpu_life as tgl


def zero_liberty_boards(s, libs):
    """bool [B]: the board holds a stone whose chain has no liberty."""
    return (((s[:, 0] | s[:, 1]) != 0) & (libs == 0)).any(axis=(1, 2))


@pytest.mark.parametrize('N', pc.SIZES)
def test_generators_give_valid_boards_and_are_deterministic(N):
    for kind in pc.SETS:
        s = pc.case(N, kind).states
        assert s.dtype == np.uint8 and s.shape == (21, 6, N, N), (N, kind)
        assert s.max() <= 1 and not (s[:, 0] & s[:, 1]).any(), (N, kind)
        for p in (2, 4, 5):
            assert (s[:, p] == s[:, p, :1, :1]).all(), (N, kind, p)
        assert ((s[:, 3] & (s[:, 0] | s[:, 1])) == (s[:, 0] | s[:, 1])).all(), (N, kind)      # a stone's point is invalid
        assert np.array_equal(s, pc.states_of(N, kind)), (N, kind)
    r, c = pc.case(N, 'random').states, pc.case(N, 'clean').states
    assert np.array_equal(r[:, 2, 0, 0], np.arange(21) % 2) and np.array_equal(c[:, 2, 0, 0], np.arange(21) % 2)
    assert not r[:, 4:].any() and not c[:, 4:].any()
    assert np.array_equal(r[:, 3], r[:, 0] | r[:, 1])                                           # plane 3 is the stones
    assert not zero_liberty_boards(c, pc.case(N, 'clean').libs).any(), N
    assert ((c[:, 0] <= r[:, 0]) & (c[:, 1] <= r[:, 1])).all(), N                               # the same stones, chains removed
    extra = (c[:, 3] & ~(c[:, 0] | c[:, 1]) & 1).sum(axis=(1, 2))
    assert np.array_equal(extra, (np.arange(21) % 3 == 0).astype(extra.dtype)), N              # one marked empty point
    assert not np.array_equal(pc.random_boards(N, seed=8), r)


@pytest.mark.parametrize('N', pc.SIZES)
def test_policy_positions_are_not_vacuous(N):
    c = pc.case(N, 'policy')
    ended = c.states[:, 5, 0, 0] != 0
    if N >= 3:
        assert ended.any() and not ended.all(), N
    if N >= 4:
        assert all(c.life[:, p].any() for p in range(4)), (N, [int(c.life[:, p].sum()) for p in range(4)])
        assert all(c.ladder[:, p].any() for p in range(4)), (N, [int(c.ladder[:, p].sum()) for p in range(4)])


@pytest.mark.parametrize('N', pc.SIZES)
def test_random_boards_are_not_vacuous(N):
    r, c = pc.case(N, 'random'), pc.case(N, 'clean')
    assert zero_liberty_boards(r.states, r.libs).any(), N
    # the rule the kernels are held to: a stone of such a chain is in no liberty class
    stones = (r.states[:, 0] | r.states[:, 1]) != 0
    assert (r.features[:, 2:10].sum(axis=1)[stones & (r.libs == 0)] == 0).all()
    if N >= 3:
        assert c.ladder[:, 0].any() or c.ladder[:, 1].any(), N
        assert c.features[:, 10].any() and (c.features[:, 10].sum(axis=(1, 2))[::3] < (c.features[:, 0] + c.features[:, 1] == 0).sum(
            axis=(1, 2))[::3]).all(), N                                                         # the marked point is not legal
    if N >= 7:
        deep = max(x['depth'] for x in c.stats)
        assert deep > max(x['depth'] for x in pc.case(N, 'policy').stats), (N, deep)


@pytest.mark.parametrize('N', pc.SIZES)
def test_expectations_agree_with_themselves_under_the_eight_orientations(N):
    o = tgl.mixed(21) & 7
    assert set(o) == set(range(8))
    for kind in pc.SETS:
        c = pc.case(N, kind)
        t = se.orient_images(c.states, o)
        assert np.array_equal(fe.batch_features(t), se.orient_images(c.features, o)), (N, kind, 'features')
        assert np.array_equal(fe.batch_group_liberties(t), se.orient_images(c.libs, o)), (N, kind, 'counts')
        assert np.array_equal(life.batch_life(t), se.orient_images(c.life, o)), (N, kind, 'life')
        if kind in pc.LADDER_SETS:
            planes, aborted = pc.oriented_ladder(N, kind, tuple(int(v) for v in tgl.mixed(21)))
            clear = c.aborted == 0
            assert 4 * int((~clear).sum()) < 21, (N, kind, int((~clear).sum()))     # the check cannot empty itself
            assert np.array_equal(planes[clear], se.orient_images(c.ladder, o)[clear]), (N, kind, 'ladder')
            assert not aborted[clear].any(), (N, kind)
