"""CPU: what tests/test_gpu_plane_scale.py relies on, without a device.  The reference that tests/plane_scale.py reads off the
oracle's children must not define itself: at every board size from 2 to 19 it equals the definitional modules
(features_expect, outcome_expect, hash_expect) on the policy and the clean set of tests/plane_cases.py, with plane 3 as given
and with plane 3 holding only the stones (ko and suicide points are candidates then).  The positions it is applied to are not
vacuous: large captures, self-ataris of large chains, ko points and finished games at every size that can hold them; and the
games of the repeat mask repeat positions with and without the planted entries."""
import numpy as np
import pytest

import hash_expect as he
import outcome_expect as oe
import plane_cases as pc
import plane_scale as ps

SETS = ('policy', 'clean')


def test_the_key_table_is_the_definitions():
    assert ps.KEYS.dtype == np.uint64 and ps.KEYS.shape == (2, 19, 19)
    assert ps.KEYS.reshape(-1).tolist() == he.KEYS


@pytest.mark.parametrize('N', pc.SIZES)
def test_the_reference_from_the_children_equals_the_definitional_modules(N):
    for kind in SETS:
        c, o, h = pc.case(N, kind), oe.case(N, kind), he.case(N, kind)
        ref = ps.reference(c.states)
        tag = (N, kind)
        assert np.array_equal(ref.cand, oe.candidates_of(c.states)), tag
        assert np.array_equal(ref.raw, o.raw[:, :3]), tag
        assert np.array_equal(ref.counts, o.counts) and np.array_equal(ref.planes, o.planes), tag
        assert np.array_equal(ref.hashes, h.hashes) and np.array_equal(ref.moves, h.moves), tag
        assert np.array_equal(ref.features, c.features) and np.array_equal(ref.libs, c.libs), tag
        # plane 3 = the stones: every empty point of a live game is a candidate, suicides and the ko point included
        opened = ps.stones_only(c.states)
        ref_open = ps.reference(opened)
        raw = oe.batch_outcome(opened)
        assert np.array_equal(ref_open.raw, raw[:, :3]), tag
        assert np.array_equal(ref_open.counts, oe.counts_of(raw)) and np.array_equal(ref_open.planes, oe.planes_of(raw)), tag
        assert np.array_equal(ref_open.moves, he.batch_move_hashes(opened)), tag
        assert (ref_open.cand & (ref_open.raw[:, 0] == 0)).any() or kind == 'policy' or N == 2, tag     # rule 4 is exercised
        ps.capture_identity(ref)


@pytest.mark.parametrize('N', ps.SIZES)
def test_the_positions_hold_what_the_kernels_can_get_wrong(N):
    c = ps.positions(N)
    B = len(c.states)
    libs, cap, size = (c.ref.raw[:, k] for k in range(3))
    ko_boards = int((c.ref.features[:, 11] != 0).reshape(B, -1).any(axis=1).sum())
    over = c.states[:, 5, 0, 0] != 0
    assert c.first == ps.batch_of(N) and c.first <= B <= c.first + ps.KO_CHILDREN
    assert over.any() and not over.all(), N                                   # finished games, and live ones
    assert not c.ref.cand[over].any() and not c.ref.raw[over].any()
    assert (c.ref.moves[over] == c.ref.hashes[over, None]).all()
    assert c.ref.cand.any() and (cap > 0).any() and (libs == 1).any(), N
    assert (c.ref_open.cand & (c.ref_open.raw[:, 0] == 0)).any(), N           # suicides, once plane 3 lets them through
    if N >= 4:
        assert int((cap >= 4).sum()) >= 50, (N, int((cap >= 4).sum()))
        assert int(((libs == 1) & (size >= 4)).sum()) >= 50, N
        assert ko_boards >= 8, (N, ko_boards)
    elif N == 3:
        assert ko_boards >= 8 and cap.max() >= 4 and size.max() >= 4, N       # (a 3x3 board holds all of these)
    else:
        assert ko_boards == 0 and 1 <= cap.max() <= 3 and size.max() <= 3, N  # four points: no ko shape, no chain of four with a liberty
    # the move planes are a function of the counts, and every one of them has elements from 4x4 on
    assert np.array_equal(c.ref.planes, oe.planes_of(c.ref.raw)), N
    if N >= 4:
        assert c.ref.planes.reshape(B, 12, -1).any(axis=(0, 2)).all(), N
        assert c.ref.features.reshape(B, 16, -1).any(axis=(0, 2)).all(), N
    # a second-generation board differs from its parent: the ko point is in plane 3 and not in the stones
    ko = c.ref.features[:, 11] != 0
    assert not (ko & ((c.states[:, 0] | c.states[:, 1]) != 0)).any() and (c.states[:, 3][ko] != 0).all()


@pytest.mark.parametrize('N', ps.GAME_SIZES)
def test_the_games_repeat_positions_with_and_without_the_planted_entries(N):
    g = ps.games(N)
    M, P = len(g.states), N * N
    assert g.history.shape == (M, g.H) and g.count.shape == (M,) and g.mask.shape == (M, P + 1)
    assert M > 1000 and (g.states[:, 5, 0, 0] == 0).all()
    assert not g.mask[:, P].any() and not g.mask[:, :P][~ps.candidates(g.states).reshape(M, P)].any()
    assert (g.mask >= g.mask_plain).all()
    assert g.mask_plain.sum() > 0, N                                          # a game came back to a position by itself
    assert (g.mask[g.planted] > g.mask_plain[g.planted]).sum() >= 50, N       # ... and by the planted entries
    assert not (g.mask[~g.planted] != g.mask_plain[~g.planted]).any()
    assert ps.counts_of(np.full(5, 7), g.H).tolist() == [7, 6, 0, g.H + 5, -1]
    assert set(np.unique(g.count[g.count <= 0]).tolist()) == {-1, 0} and (g.count == g.H + 5).any()
    # a sample of rows against the definitional, hash-based mask: 64-bit hashes of a few thousand positions do not collide
    rows = np.unique(np.concatenate([np.flatnonzero(g.mask.any(axis=1))[:40], np.arange(0, M, max(1, M // 40))]))
    moves = he.batch_move_hashes(g.states[rows])
    assert np.array_equal(he.batch_repeat(g.states[rows], moves, g.history[rows], g.count[rows]), g.mask[rows]), N
    assert np.array_equal(g.history[rows, 0], np.zeros(len(rows), np.int64))  # every game starts from the empty board
