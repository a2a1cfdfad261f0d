"""CPU: the pass-alive life planes (gogame.batch_life / batch_life_tracked / batch_settled, gg_batch_life*) without a device -
the expectation module (life_expect) on hand-worked positions with the expected arrays written out, the property that ended
policy games are settled, and the argument checks of the C entry points and the Python API."""
import numpy as np
import pytest

import features_expect as fe
import life_expect as le
import mc_expect as mc
import mc_policy_expect as mp


@pytest.fixture(scope='module')
def built(native_built):
    from gymgo_amd import _lib
    return _lib


def grid(*rows):
    """uint8 [N, N] from strings of digits ('.' = 0)."""
    return np.array([[0 if ch == '.' else int(ch) for ch in row] for row in rows], np.uint8)


def pad(rows, N):
    """rows, filled up with empty rows to N."""
    return list(rows) + ['.' * N] * (N - len(rows))


def check(rows, alive=(), safe=(), opp_alive=(), opp_safe=(), settled=0):
    """The position `rows` (black = X) in all four forms: black / white to move, and with the colours swapped.  alive / safe:
    the expected planes of X, opp_alive / opp_safe: of O, as the leading rows of the grid (the rest is zero)."""
    N = len(rows)
    x_alive, x_safe, o_alive, o_safe = (grid(*pad(g, N)) for g in (alive, safe, opp_alive, opp_safe))
    for swapped in (False, True):
        for white_to_move in (False, True):
            s = fe.board(le.swap(rows) if swapped else rows, white_to_move=white_to_move)
            got = le.life(s)
            assert got.shape == (4, N, N) and got.dtype == np.uint8
            x_is_own = swapped == white_to_move        # X is black unless swapped; own is black unless white moves
            want = [x_alive, o_alive, x_safe, o_safe] if x_is_own else [o_alive, x_alive, o_safe, x_safe]
            for p in range(4):
                assert np.array_equal(got[p], want[p]), (rows, swapped, white_to_move, le.NAMES[p], got[p], want[p])
            assert le.settled(s[None])[0] == settled


def test_two_eyes_in_the_corner_live_one_eye_does_not():
    check(pad(['.X.X.', 'XXXX.'], 5), alive=['.1.1.', '1111.'], safe=['1.1..'])
    check(pad(['.XX..', 'XXX..'], 5))


def test_two_chains_that_share_their_only_two_eyes_both_live():
    # the stone at (0, 0) and the chain around it: (0, 1) and (1, 0) are vital to both
    check(pad(['X.X..', '.XX..', 'XX...'], 5), alive=['1.1..', '.11..', '11...'], safe=['.1...', '1....'])


def test_an_eye_holding_an_opponent_stone_beside_its_empty_point_is_vital():
    check(pad(['.OX.X', 'XXXXX'], 5), alive=['..1.1', '11111'], safe=['11.1.'])


def test_bent_three_and_square_four_eyes_whose_points_all_touch_the_chain():
    # the middle point (0, 2) of the bent eye touches (0, 3)
    check(pad(['X..X.X.', 'XX.XXX.', '.XXX...'], 7), alive=['1..1.1.', '11.111.', '.111...'], safe=['.11.1..', '..1....'])
    check(pad(['X..X.X.', 'X..XXX.', 'XXXX...'], 7), alive=['1..1.1.', '1..111.', '1111...'], safe=['.11.1..', '.11....'])


def test_a_large_eye_with_an_interior_point_that_touches_no_stone_is_not_vital():
    # (0, 0) of the 2x2 corner eye touches nothing: one vital region is not enough
    check(pad(['..X.X..', '..XXX..', 'XXX....'], 7))
    # ... and a lone stone of the same colour on that point does not help: the stone has no vital region and is dropped, then
    # the region that borders it
    check(pad(['X.X.X..', '..XXX..', 'XXX....'], 7))


def test_a_false_eye_at_the_edge_takes_the_group_with_it():
    # (0, 2) is closed by the lone stone (0, 3), which has no second region: it is dropped, then the region it borders,
    # then the group - Benson's iteration at its shortest
    rows = pad(['.X.X.', 'XXX..'], 5)
    check(rows)
    assert le.iterations(fe.board(rows)) == 2
    # the stone connected: a real eye
    check(pad(['.X.XX', 'XXXXX'], 5), alive=['.1.11', '11111'], safe=['1.1..'])


def test_cascade_dies_one_chain_per_iteration():
    for N, length in ((9, 3), (19, 6)):
        rows, L = le.cascade(N, False)
        assert L == length
        s = fe.board(rows)
        got = le.life(s)
        assert np.array_equal(got[0], s[0]) and not got[1].any() and not got[3].any()     # every black chain lives
        dying, _ = le.cascade(N, True)
        d = fe.board(dying)
        assert not le.life(d).any() and le.iterations(d) == L
        assert le.settled(np.stack([s, d])).tolist() == [0, 0]
    # the 9x9 board, written out
    rows, _ = le.cascade(9, False)
    assert rows == ['.X.XXXXXX',
                    'XXXXXXOOO',
                    'OOOOOO.XX',
                    'XXXXXXX.X',
                    'OOOXXXXXX',
                    'XX.OOOOOO',
                    'X.XXXXXXX',
                    'XXXXXXXX.',
                    '.........']
    check(rows,
          alive=['.1.111111', '111111...', '.......11', '1111111.1', '...111111', '11.......', '1.1111111', '11111111.'],
          safe=['1.1......', '......111', '1111111..', '.......1.', '111......', '..1111111', '.1.......'])


def test_empty_board_one_stone_full_boards_and_2x2():
    check(['.....'] * 5)
    check(pad(['.....', '..X..'], 5))
    check(['XXXXX', 'XXOXX', 'XOOOX', 'XXOXX', 'XXXXX'])              # no empty point: nothing is vital
    check(['XX', 'XX'])
    check(['X.', '..'])
    check(['XO', 'O.'])
    check(['X.', '.X'], alive=['1.', '.1'], safe=['.1', '1.'], settled=1)   # two stones, two shared eyes


def test_settled_boards():
    # both colours alive, every other point an eye
    check(['.X.X.', 'XXXXX', 'OOOOO', 'OOOOO', '.O.O.'], alive=['.1.1.', '11111'], safe=['1.1.1'],
          opp_alive=['.....', '.....', '11111', '11111', '.1.1.'], opp_safe=['.....', '.....', '.....', '.....', '1.1.1'], settled=1)
    # one neutral point left
    check(['.X.X.', 'XXXXX', '.....', 'OOOOO', '.O.O.'], alive=['.1.1.', '11111'], safe=['1.1.1'],
          opp_alive=['.....', '.....', '.....', '11111', '.1.1.'], opp_safe=['.....', '.....', '.....', '.....', '1.1.1'])
    # dead stones inside an eye are the owner's safe points
    check(['.OX.X', 'XXXXX', 'OOOOO', 'OOOOO', '.O.O.'], alive=['..1.1', '11111'], safe=['11.1.'],
          opp_alive=['.....', '.....', '11111', '11111', '.1.1.'], opp_safe=['.....', '.....', '.....', '.....', '1.1.1'], settled=1)


def test_orientation_of_the_expectation():
    s = fe.board(pad(['.X.X.', 'XXXX.'], 5))
    p = le.batch_life(np.stack([s] * 8))
    o = le.oriented(p, np.arange(8))
    assert np.array_equal(o[0], p[0]) and np.array_equal(o[1], p[0][..., ::-1]) and np.array_equal(o[2], p[0][..., ::-1, :])
    import symmetry_expect as se
    for k in range(8):   # the planes of the turned position
        turned = se.orient_image(s, k)
        assert np.array_equal(le.life(turned), o[k])


@pytest.mark.parametrize('N', [5, 9])
def test_every_ended_policy_game_is_settled(N):
    B = 64
    states, _, _, _ = mp.policy_rollout(np.zeros((B, 6, N, N), np.uint8), mc.po_seed(7, np.arange(B)), 2 * N * N)
    ended = states[:, 5, 0, 0] != 0
    assert ended.sum() >= 16
    assert le.settled(states[ended]).all()


def test_entry_points_check_arguments_without_device(built):
    L = built.lib()
    for name in ('gg_life_planes', 'gg_batch_life', 'gg_batch_life_tracked'):
        assert name in built.EXPORTS and name in built._SIGNATURES and getattr(L, name)
    assert L.gg_life_planes() == 4
    p = 16
    for fn in (L.gg_batch_life, L.gg_batch_life_tracked):
        # 1. sizes and the dtype - before anything else
        assert fn(None, None, None, None, 3, 4, 20, None) == -1 and fn(p, None, p, None, 3, 4, 1, None) == -1
        assert fn(p, None, p, None, 3, -1, 9, None) == -1
        assert fn(None, None, None, None, 4, 4, 9, None) == -1 and fn(p, None, p, None, -1, 4, 9, None) == -1
        # 2. B = 0 is no work, whatever the pointers
        for dt in range(4):
            assert fn(None, None, None, None, dt, 0, 9, None) == 0
        assert fn(None, None, None, None, 4, 0, 9, None) == -1
        # 3. the input and out
        assert fn(None, None, p, None, 3, 4, 9, None) == -2 and fn(p, None, None, None, 3, 4, 9, None) == -2
        assert fn(None, None, p + 1, None, 2, 4, 9, None) == -2                         # (before the alignment)
        # 4. out aligned to its element
        assert fn(p, None, p + 1, None, 2, 4, 9, None) == -3 and fn(p, None, p + 1, None, 1, 4, 9, None) == -3
        assert fn(p, None, p + 2, None, 0, 4, 9, None) == -3 and fn(p, p, p + 3, p, 0, 4, 19, None) == -3


def test_python_api_checks_arguments_before_a_device_is_touched():
    import torch
    from gymgo_amd import gogame
    assert gogame.LIFE_PLANES == 4 and gogame.LIFE_NAMES == le.NAMES
    st = np.zeros((2, 6, 5, 5), np.uint8)
    tr = torch.zeros((2, 26), dtype=torch.int32)
    for bad in (torch.float64, torch.int8, torch.bool, np.float16, 'float16', None):
        with pytest.raises(ValueError):
            gogame.batch_life(st, dtype=bad)
        with pytest.raises(ValueError):
            gogame.life(st[0], dtype=bad)
        with pytest.raises(ValueError):
            gogame.batch_life_tracked(tr, dtype=bad)
    for out in (torch.zeros((2, 4, 5, 5), dtype=torch.float16), torch.zeros((2, 4, 5, 4), dtype=torch.float16), np.zeros((2, 4, 5, 5)),
                torch.zeros((2, 4, 5, 5), dtype=torch.float32)):
        with pytest.raises(ValueError):
            gogame.batch_life(st, dtype=torch.float16, out=out)
        with pytest.raises(ValueError):
            gogame.batch_life_tracked(tr, dtype=torch.float16, out=out)
    with pytest.raises(ValueError):
        gogame.batch_life(np.zeros((2, 5, 5, 5), np.uint8))
    with pytest.raises(ValueError):
        gogame.batch_settled(np.zeros((2, 6, 5, 4), np.uint8))
    with pytest.raises(ValueError):
        gogame.batch_life(st, dtype=torch.bfloat16)              # NumPy in, NumPy out: there is no NumPy bfloat16
    with pytest.raises(ValueError):
        gogame.life(st[0], dtype=torch.bfloat16)
    for orient in ([0, 1, 2], np.zeros(2, np.float32), torch.zeros(2, dtype=torch.bool)):
        with pytest.raises(ValueError):
            gogame.batch_life(st, orient=orient)
        with pytest.raises(ValueError):
            gogame.batch_life_tracked(tr, orient=orient)
    with pytest.raises(ValueError):
        gogame.batch_life_tracked(torch.zeros((2, 27), dtype=torch.int32))


def test_life_has_no_cpu_fallback(built):
    import torch
    from gymgo_amd import gogame
    if torch.cuda.is_available():
        pytest.skip('device present')
    st = np.zeros((2, 6, 9, 9), np.uint8)
    for call in (lambda: gogame.batch_life(st), lambda: gogame.life(st[0]), lambda: gogame.batch_settled(st),
                 lambda: gogame.batch_life_tracked(torch.zeros((2, 46), dtype=torch.int32))):
        with pytest.raises(built.GymGoNativeError):
            call()


def test_life_needs_features_and_refuses_the_playout_evaluator(monkeypatch):
    import torch
    from gymgo_amd import gogame
    monkeypatch.setattr(gogame, '_device', lambda: torch.device('cpu'))
    empty = np.zeros((0, 6, 5, 5), np.uint8)
    p, v = np.zeros((0, 26), np.float32), np.zeros(0, np.float32)
    ev3 = lambda planes, legal, life: (p, v)
    for call in (lambda: gogame.PuctSearch(empty, 2, life=True),
                 lambda: gogame.batch_puct(empty, 2, ev3, life=True),
                 lambda: gogame.puct_actions(empty, 2, ev3, life=True),
                 lambda: gogame.puct(np.zeros((6, 5, 5), np.uint8), 2, ev3, life=True),
                 lambda: gogame.puct_play(empty, 1, 2, ev3, life=True),
                 lambda: gogame.puct_selfplay(empty, 1, 2, ev3, life=True)):
        with pytest.raises(ValueError, match='features'):
            call()
    ev = gogame.playout_evaluator(2, komi=0.0)
    for call in (lambda: gogame.batch_puct(empty, 2, ev, features=torch.float16, life=True),
                 lambda: gogame.puct_play(empty, 1, 2, ev, features=torch.uint8, life=True),
                 lambda: gogame.puct_selfplay(empty, 1, 2, ev, features=torch.float32, life=True)):
        with pytest.raises(ValueError, match='needs states'):
            call()


def test_life_on_no_roots_hands_out_empty_planes(monkeypatch):
    import torch
    from gymgo_amd import gogame
    monkeypatch.setattr(gogame, '_device', lambda: torch.device('cpu'))
    empty = np.zeros((0, 6, 5, 5), np.uint8)
    A = 26
    p, v = np.zeros((0, A), np.float32), np.zeros(0, np.float32)
    for leaves in (None, 3):
        for symmetry in (None, 5):
            s = gogame.PuctSearch(empty, 2, leaves=leaves, features=torch.bfloat16, symmetry=symmetry, life=True)
            planes, legal, life = s.select()
            assert tuple(planes.shape) == (0, 16, 5, 5) and tuple(legal.shape) == (0, A)
            assert tuple(life.shape) == (0, 4, 5, 5) and life.dtype == torch.bfloat16
            s.backup(p, v)
        # life=False: two values, as ever
        assert len(gogame.PuctSearch(empty, 2, leaves=leaves, features=torch.float16).select()) == 2
        seen = []

        def ev(x, l, life):
            seen.append((tuple(x.shape), tuple(life.shape), life.dtype))
            return p, v

        gogame.batch_puct(empty, 3, ev, leaves=leaves, features=torch.float16, life=True)
        assert seen == [((0, 16, 5, 5), (0, 4, 5, 5), torch.float16)] * 3
        rec = gogame.puct_selfplay(empty, 0, 2, ev, leaves=leaves, features=torch.float16, life=True)
        assert rec.actions.shape == (0, 0)
        assert gogame.puct_play(empty, 2, 2, ev, leaves=leaves, features=torch.float16, life=True)[0].shape == (0, 2)


def test_documents_name_the_life_entry_points():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'INTEGRATION.md')).read()
    for name in ('gg_life_planes', 'gg_batch_life', 'gg_batch_life_tracked'):
        assert name in text, name
