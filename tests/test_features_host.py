"""CPU: the network input planes (gogame.batch_features / batch_features_tracked / batch_group_liberties, gg_batch_features*)
without a device - the expectation module (features_expect) on hand-worked positions with the expected arrays written out,
its legal / ko planes against the NumPy oracle on the golden games, and the argument checks of the C entry points and the
Python API."""
import numpy as np
import pytest

import features_expect as fe
from oracle import np_oracle


@pytest.fixture(scope='module')
def built(native_built):
    from gymgo_amd import _lib
    return _lib


def grid(*rows):
    """uint8 [N, N] from strings of digits ('.' = 0)."""
    return np.array([[0 if ch == '.' else int(ch) for ch in row] for row in rows], np.uint8)


def check_planes(state, want):
    """want: {plane: grid}; every plane that is not named is all zero."""
    got = fe.features(state)
    N = state.shape[-1]
    assert got.shape == (16, N, N) and got.dtype == np.uint8
    for p in range(16):
        w = want.get(p, np.zeros((N, N), np.uint8))
        assert np.array_equal(got[p], w), (fe.NAMES[p], got[p], w)


ONES5 = grid('11111', '11111', '11111', '11111', '11111')
ONES3 = grid('111', '111', '111')


def test_lone_corner_edge_and_centre_stone():
    rows = ['X....',
            '.....',
            'X.X..',
            '.....',
            '.....']
    s = fe.board(rows)
    assert np.array_equal(fe.group_liberties(s), grid('2....', '.....', '3.4..', '.....', '.....'))
    stones = grid('1....', '.....', '1.1..', '.....', '.....')
    empty = grid('.1111', '11111', '.1.11', '11111', '11111')
    check_planes(s, {0: stones, 3: grid('1....', '.....', '.....', '.....', '.....'), 4: grid('.....', '.....', '1....', '.....', '.....'),
                     5: grid('.....', '.....', '..1..', '.....', '.....'), 10: empty, 13: ONES5, 15: ONES5})
    # white to move: the same stones are the opponent's - planes 0 / 1 and 2-5 / 6-9 swap, plane 13 is zero
    check_planes(fe.board(rows, white_to_move=True),
                 {1: stones, 7: grid('1....', '.....', '.....', '.....', '.....'), 8: grid('.....', '.....', '1....', '.....', '.....'),
                  9: grid('.....', '.....', '..1..', '.....', '.....'), 10: empty, 15: ONES5})


def test_two_groups_sharing_a_liberty():
    s = fe.board(['X.X', '...', '...'])
    assert np.array_equal(fe.group_liberties(s), grid('2.2', '...', '...'))    # (0, 1) counts for both
    check_planes(s, {0: grid('1.1', '...', '...'), 3: grid('1.1', '...', '...'), 10: grid('.1.', '111', '111'), 13: ONES3, 15: ONES3})
    # ... and of two colours
    s = fe.board(['X.O', '...', '...'])
    check_planes(s, {0: grid('1..', '...', '...'), 1: grid('..1', '...', '...'), 3: grid('1..', '...', '...'),
                     7: grid('..1', '...', '...'), 10: grid('.1.', '111', '111'), 13: ONES3, 15: ONES3})


def test_stone_in_atari_next_to_a_capturing_point_pass_and_end():
    rows = ['OX.', '...', '...']
    s = fe.board(rows)
    assert np.array_equal(fe.group_liberties(s), grid('12.', '...', '...'))
    want = {0: grid('.1.', '...', '...'), 1: grid('1..', '...', '...'), 3: grid('.1.', '...', '...'), 6: grid('1..', '...', '...'),
            10: grid('..1', '111', '111'), 12: grid('...', '1..', '...'), 13: ONES3, 15: ONES3}
    check_planes(s, want)
    # the previous move was a pass: plane 14, nothing else
    check_planes(fe.board(rows, passed=True), {**want, 14: ONES3})
    # the game has ended: planes 10 - 12 are zero
    ended = {**want, 14: ONES3}
    del ended[10], ended[12]
    check_planes(fe.board(rows, passed=True, done=True), ended)


def test_ko_against_suicide_white_to_move():
    # black has just taken at (1, 2): (1, 1) is the ko point; (0, 0), (2, 0) and (4, 0) are suicide for white
    rows = ['.XO..',
            'X.XO.',
            '.XO..',
            'X....',
            '.X...']
    s = fe.board(rows, white_to_move=True, invalid=[(1, 1), (0, 0), (2, 0), (4, 0)])
    assert np.array_equal(fe.group_liberties(s), grid('.21..', '3.13.', '.32..', '3....', '.3...'))
    check_planes(s, {0: grid('..1..', '...1.', '..1..', '.....', '.....'),
                     1: grid('.1...', '1.1..', '.1...', '1....', '.1...'),
                     2: grid('..1..', '.....', '.....', '.....', '.....'),
                     3: grid('.....', '.....', '..1..', '.....', '.....'),
                     4: grid('.....', '...1.', '.....', '.....', '.....'),
                     6: grid('.....', '..1..', '.....', '.....', '.....'),
                     7: grid('.1...', '.....', '.....', '.....', '.....'),
                     8: grid('.....', '1....', '.1...', '1....', '.1...'),
                     10: grid('...11', '....1', '...11', '.1111', '..111'),
                     11: grid('.....', '.1...', '.....', '.....', '.....'),
                     15: ONES5})
    assert fe.features(s)[11].sum() == 1 and fe.features(s)[12].sum() == 0


def replay(size, moves):
    s = np.zeros((6, size, size), np.uint8)
    for m in moves:
        s = np_oracle.next_state(s, size * size if m is None else m[0] * size + m[1]).astype(np.uint8)
    return s


def test_legal_plane_is_the_oracles_valid_moves_on_the_golden_games(golden):
    z = golden('random_games')
    games = sorted(k[:-len('/actions')] for k in z.keys() if k.endswith('/actions'))
    assert games
    n = 0
    for g in games:
        size = z[g + '/sample_states'].shape[-1]
        s = np.zeros((6, size, size), np.uint8)
        for a in z[g + '/actions']:
            f = fe.features(s)
            done = bool(s[5, 0, 0])
            assert np.array_equal(f[10], (1 - s[3]) * (0 if done else 1)), (g, n)
            assert not (f[11] & f[10]).any() and not (f[12] & ~f[10]).any()
            n += 1
            if done:
                break
            s = np_oracle.next_state(s, int(a)).astype(np.uint8)
    assert n > 100


def test_ko_plane_on_the_golden_ko_cases(scripted_cases):
    by_name = {c['name']: c for c in scripted_cases}
    for name in ('ko_protection', 'ko_wall_protection'):
        c = by_name[name]
        s = replay(c['size'], c['moves'])
        f = fe.features(s)
        (y, x), = c['then_raises']
        assert f[11].sum() == 1 and f[11, y, x] == 1 and f[12, y, x] == 0, name
    for name in ('group_kill_no_ko', 'valid_no_liberty_capture'):
        c = by_name[name]
        s = replay(c['size'], c['moves'])
        f = fe.features(s)
        assert not f[11].any(), name
        (y, x), = c['continue']
        assert f[12, y, x] == 1, name        # the capture that is allowed


def test_entry_points_check_arguments_without_device(built):
    L = built.lib()
    for name in ('gg_feature_planes', 'gg_batch_group_liberties', 'gg_batch_features', 'gg_batch_features_tracked'):
        assert name in built.EXPORTS and name in built._SIGNATURES and getattr(L, name)
    assert L.gg_feature_planes() == 16
    p = 16
    assert L.gg_batch_group_liberties(None, None, 4, 9, None) == -2
    assert L.gg_batch_group_liberties(p, None, 4, 9, None) == -2
    assert L.gg_batch_group_liberties(p, p, 4, 20, None) == -1
    assert L.gg_batch_group_liberties(None, None, 0, 9, None) == 0
    for fn in (L.gg_batch_features, L.gg_batch_features_tracked):
        assert fn(None, None, 2, 4, 9, None) == -2
        assert fn(p, None, 2, 4, 9, None) == -2
        assert fn(p, p, 2, 4, 20, None) == -1 and fn(p, p, 2, 4, 1, None) == -1 and fn(p, p, 2, -1, 9, None) == -1
        assert fn(p, p, 4, 4, 9, None) == -1 and fn(p, p, -1, 4, 9, None) == -1
        for dt in range(4):
            assert fn(None, None, dt, 0, 9, None) == 0


def test_python_api_checks_arguments_before_a_device_is_touched():
    import torch
    from gymgo_amd import gogame
    assert gogame.FEATURE_PLANES == 16 and len(gogame.FEATURE_NAMES) == 16 and gogame.FEATURE_NAMES == fe.NAMES
    st = np.zeros((2, 6, 5, 5), np.uint8)
    tr = torch.zeros((2, 26), dtype=torch.int32)
    for bad in (torch.float64, torch.int8, torch.bool, np.float16, 'float16', None):
        with pytest.raises(ValueError):
            gogame.batch_features(st, dtype=bad)
        with pytest.raises(ValueError):
            gogame.features(st[0], dtype=bad)
        with pytest.raises(ValueError):
            gogame.batch_features_tracked(tr, dtype=bad)
        with pytest.raises(ValueError):
            gogame.PuctSearch(st, 2, features=bad) if bad is not None else gogame.batch_features(st, dtype=bad)
    # out: a host tensor, a wrong shape, a wrong dtype
    for out in (torch.zeros((2, 16, 5, 5), dtype=torch.float16), torch.zeros((2, 16, 5, 4), dtype=torch.float16), np.zeros((2, 16, 5, 5)),
                torch.zeros((2, 16, 5, 5), dtype=torch.float32)):
        with pytest.raises(ValueError):
            gogame.batch_features(st, dtype=torch.float16, out=out)
        with pytest.raises(ValueError):
            gogame.batch_features_tracked(tr, dtype=torch.float16, out=out)
    with pytest.raises(ValueError):
        gogame.batch_features(np.zeros((2, 5, 5, 5), np.uint8))
    with pytest.raises(ValueError):
        gogame.batch_group_liberties(np.zeros((2, 6, 5, 4), np.uint8))
    with pytest.raises(ValueError):
        gogame.batch_features(st, dtype=torch.bfloat16)          # NumPy in, NumPy out: there is no NumPy bfloat16


def test_features_have_no_cpu_fallback(built):
    import torch
    from gymgo_amd import gogame
    if torch.cuda.is_available():
        pytest.skip('device present')
    st = np.zeros((2, 6, 9, 9), np.uint8)
    for call in (lambda: gogame.batch_features(st), lambda: gogame.features(st[0]), lambda: gogame.batch_group_liberties(st),
                 lambda: gogame.group_liberties(st[0]),
                 lambda: gogame.batch_features_tracked(torch.zeros((2, 46), dtype=torch.int32))):
        with pytest.raises(built.GymGoNativeError):
            call()


def test_playout_evaluator_is_refused_with_features(monkeypatch):
    import torch
    from gymgo_amd import gogame
    monkeypatch.setattr(gogame, '_device', lambda: torch.device('cpu'))
    empty = np.zeros((0, 6, 5, 5), np.uint8)
    ev = gogame.playout_evaluator(2, komi=0.0)
    assert ev.needs_states is True
    for call in (lambda: gogame.batch_puct(empty, 2, ev, features=torch.float16),
                 lambda: gogame.puct_play(empty, 1, 2, ev, features=torch.uint8),
                 lambda: gogame.puct_selfplay(empty, 1, 2, ev, features=torch.float32)):
        with pytest.raises(ValueError, match='needs states'):
            call()
    # any other evaluator is taken as it is
    p, v = np.zeros((0, 26), np.float32), np.zeros(0, np.float32)
    assert gogame.batch_puct(empty, 2, lambda planes, legal: (p, v), features=torch.float16).visits.shape == (0, 26)


def test_features_none_is_the_search_as_before_and_a_dtype_hands_out_planes(monkeypatch):
    import torch
    from gymgo_amd import gogame
    monkeypatch.setattr(gogame, '_device', lambda: torch.device('cpu'))
    empty = np.zeros((0, 6, 5, 5), np.uint8)
    A = 26
    p, v = np.zeros((0, A), np.float32), np.zeros(0, np.float32)
    for leaves in (None, 3):
        s = gogame.PuctSearch(empty, 2, leaves=leaves)
        assert s._feat is None and not hasattr(s, '_planes')
        states, legal = s.select()
        assert tuple(states.shape) == (0, 6, 5, 5) and states.dtype == torch.uint8 and tuple(legal.shape) == (0, A)
        s.backup(p, v)
        s = gogame.PuctSearch(empty, 2, leaves=leaves, features=torch.bfloat16)
        planes, legal = s.select()
        assert tuple(planes.shape) == (0, 16, 5, 5) and planes.dtype == torch.bfloat16 and tuple(legal.shape) == (0, A)
        s.backup(p, v)
        seen = []

        def ev(x, l):
            seen.append((tuple(x.shape), x.dtype))
            return p, v

        gogame.batch_puct(empty, 3, ev, leaves=leaves, features=torch.float16)
        assert seen == [((0, 16, 5, 5), torch.float16)] * 3
        rec = gogame.puct_selfplay(empty, 0, 2, ev, leaves=leaves, features=torch.float16)
        assert rec.actions.shape == (0, 0)


def test_documents_name_the_feature_entry_points():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'INTEGRATION.md')).read()
    for name in ('gg_feature_planes', 'gg_batch_group_liberties', 'gg_batch_features', 'gg_batch_features_tracked', 'GG_FEAT_U8'):
        assert name in text, name
