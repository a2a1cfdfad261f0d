"""CPU: what tests/test_gpu_outcome.py relies on, without a device.  The expectation of the move-outcome planes
(tests/outcome_expect.py) is held against two independent sources at every board size from 2 to 19 - the children the C
restatement plays (the captured stones) and the per-group liberty counts of features_expect on those children (the
liberties afterwards) -, against the capture plane of features_expect, and it is not vacuous on the sets the GPU test
runs: every plane has elements, some candidate joins two own chains and captures, the clean boards hold suicides.  The
hand-made boards show the counts they were drawn for."""
import numpy as np
import pytest

import features_expect as fe
import outcome_expect as oe
import plane_cases as pc

SETS = ('policy', 'clean')


@pytest.mark.parametrize('N', pc.SIZES)
def test_counts_agree_with_the_children_of_the_policy_positions(N):
    """(a) captured = the opponent stones the child has lost, libs = the liberty count of the played stone's group there."""
    from oracle import c_oracle
    c = oe.case(N, 'policy')
    children = c_oracle.batch_children(c.states)
    seen = 0
    for b, s in enumerate(c.states):
        white = int(s[2, 0, 0])
        opp = 0 if white else 1
        cand = oe.candidates(s)
        assert np.array_equal(cand, fe.features(s)[10] != 0), (N, b)            # the legal plane
        for y, x in np.argwhere(cand):
            child = children[b, y * N + x]
            assert child[white, y, x] == 1 and child[2, 0, 0] != white, (N, b, y, x)
            assert c.raw[b, 1, y, x] == int(s[opp].sum()) - int(child[opp].sum()), (N, b, y, x)
            assert min(c.raw[b, 0, y, x], 255) == fe.group_liberties(child)[y, x], (N, b, y, x)
            assert c.raw[b, 2, y, x] >= 1
            seen += 1
    assert seen or N == 2, N


@pytest.mark.parametrize('N', pc.SIZES)
def test_captures_exactly_on_the_capture_plane(N):
    """(b) captured > 0 exactly where plane 12 of the feature planes is set - also on the clean boards, where a candidate
    need not be a legal move."""
    for kind in SETS:
        c = oe.case(N, kind)
        assert np.array_equal(c.raw[:, 1] > 0, pc.case(N, kind).features[:, 12] != 0), (N, kind)


@pytest.mark.parametrize('N', pc.SIZES)
def test_the_sets_are_not_vacuous(N):
    """(c) over the policy and the clean set together."""
    policy, clean = oe.case(N, 'policy'), oe.case(N, 'clean')
    per_plane = policy.planes.sum(axis=(0, 2, 3)) + clean.planes.sum(axis=(0, 2, 3))
    if N >= 5:      # (4x4 has no capture of exactly three)
        assert (per_plane > 0).all(), (N, per_plane)
    joins = sum(int(((c.raw[:, 3] >= 2) & (c.raw[:, 1] > 0)).sum()) for c in (policy, clean))
    if N >= 3:
        assert joins > 0, N
    suicides = [int((oe.candidates_of(c.states) & (c.raw[:, 0] == 0)).sum()) for c in (policy, clean)]
    assert suicides[0] == 0 and suicides[1] > 0, (N, suicides)
    assert clean.states[:, 2, 0, 0].any() and not clean.states[:, 2, 0, 0].all()   # both colours move


def test_figures_at_19():
    """The element counts at N = 19 that the pull request's description quotes."""
    policy, clean = oe.case(19, 'policy'), oe.case(19, 'clean')
    assert policy.planes.sum(axis=(0, 2, 3)).tolist() == [136, 219, 314, 858, 47, 13, 4, 12, 86, 23, 6, 21]
    assert clean.planes.sum(axis=(0, 2, 3)).tolist() == [171, 408, 895, 2446, 74, 5, 10, 2, 128, 15, 9, 19]
    assert [int(((c.raw[:, 3] >= 2) & (c.raw[:, 1] > 0)).sum()) for c in (policy, clean)] == [18, 22]
    assert int((oe.candidates_of(clean.states) & (clean.raw[:, 0] == 0)).sum()) == 51


def test_crafted_boards_show_what_they_were_drawn_for():
    """(d)"""
    names = [name for name, _, _ in oe.CRAFTED]
    for word in ('snapback', 'join', 'corner', 'edge', 'ko point', 'suicide', 'ended', 'white', 'more than 255 stones played',
                 'capture of more than 255'):
        assert any(word in n for n in names), word
    for name, s, checks in oe.CRAFTED:
        stones = (s[0] | s[1]) != 0
        assert (fe.group_liberties(s)[stones] > 0).all(), name           # the contract's premise
        raw = oe.outcome(s)
        for y, x, want in checks:
            assert tuple(int(v) for v in raw[:3, y, x]) == want, (name, y, x)
    by = {name: (s, oe.outcome(s)) for name, s, _ in oe.CRAFTED}
    s, raw = by['snapback, white to move']
    assert s[2, 0, 0] == 1 and oe.planes_of(raw)[[0, 4, 11], 0, 3].all()
    s, raw = by['join two chains and capture']
    assert raw[3, 1, 2] == 2 and raw[1, 1, 2] == 1 and raw[0, 1, 2] == 1     # the captured point is the joined chain's liberty
    assert not by['an ended game'][1].any()
    s, raw = by['the ko point marked in plane 3']
    assert s[3, 1, 2] == 1 and fe.features(s)[11, 1, 2] == 1 and not raw[:, 1, 2].any()
    s, raw = by['a suicide with plane 3 clear']
    assert oe.candidates(s)[0, 0] and not raw[:3, 0, 0].any()
    # the saturation: the counts say 255 where the numbers are larger, the planes say ">= 4"
    s, raw = by['a chain of more than 255 stones played into']
    assert raw[2, 0, 0] == 323 and oe.counts_of(raw)[2, 0, 0] == 255 and oe.planes_of(raw)[3, 0, 0] == 1
    s, raw = by['a capture of more than 255 stones']
    assert raw[1, 0, 0] == 322 and oe.counts_of(raw)[1, 0, 0] == 255 and oe.planes_of(raw)[7, 0, 0] == 1


def test_planes_follow_from_the_counts():
    raw = np.zeros((4, 1, 6), int)
    raw[0, 0] = [0, 1, 1, 2, 3, 9]
    raw[1, 0] = [0, 0, 2, 3, 4, 1]
    raw[2, 0] = [0, 1, 7, 2, 3, 300]
    p = oe.planes_of(raw)[:, 0]
    assert p[:4].T.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    assert p[4:8].T.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 0, 0, 0]]
    assert p[8:].T.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert oe.counts_of(raw)[2, 0].tolist() == [0, 1, 7, 2, 3, 255]
