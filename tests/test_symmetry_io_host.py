"""CPU: the symmetry-aware network I/O (gg_batch_features_oriented / gg_batch_features_tracked_oriented,
gg_batch_symmetry_policy, gg_batch_draw_orient; gogame.batch_features(orient=), batch_symmetry_policy, batch_draw_orient,
PuctSearch(symmetry=), selfplay_batch) without a device: the expectation module (symmetry_expect) against
gogame.symmetry_actions, the draw's frequencies, the symbols, the argument checks of the C entry points in their documented
order, the ValueErrors of the Python calls, and selfplay_batch's value targets on a hand-written record."""
import numpy as np
import pytest

import symmetry_expect as se

NEW = ('gg_batch_features_oriented', 'gg_batch_features_tracked_oriented', 'gg_batch_symmetry_policy', 'gg_batch_draw_orient')


@pytest.fixture(scope='module')
def built(native_built):
    from gymgo_amd import _lib
    return _lib


@pytest.mark.parametrize('N', (2, 3, 5, 9, 19))
def test_action_tables(N):
    import torch
    from gymgo_amd import gogame
    A = N * N + 1
    fwd, inv = se.action_tables(N)
    ident = np.arange(A)
    assert np.array_equal(fwd[0], ident) and np.array_equal(inv[0], ident)          # orientation 0 is the identity
    for o in range(8):
        assert np.array_equal(inv[o][fwd[o]], ident) and np.array_equal(fwd[o][inv[o]], ident)   # forward then inverse
        assert sorted(fwd[o]) == list(ident)
        assert fwd[o, A - 1] == A - 1 and inv[o, A - 1] == A - 1                     # the pass is fixed
        got = gogame.symmetry_actions(torch.arange(A), torch.full((A,), o), N).numpy()
        assert np.array_equal(got, fwd[o]), o                                       # symmetry_actions on every action
    assert N == 2 or len({tuple(f) for f in fwd}) == 8
    # turn_policy is the image rule on the first N * N elements
    p = np.arange(8 * A, dtype=np.int32).reshape(8, A)
    view = se.turn_policy(p, np.arange(8))
    for o in range(8):
        assert np.array_equal(view[o, :-1].reshape(N, N), se.orient_image(p[o, :-1].reshape(N, N), o)) and view[o, -1] == p[o, -1]
    assert np.array_equal(se.turn_policy(view, np.arange(8), inverse=True), p)


def test_orient_image_is_the_reference_composition():
    x = np.arange(2 * 9).reshape(2, 3, 3)
    assert np.array_equal(se.orient_image(x, 0), x)
    assert np.array_equal(se.orient_image(x, 1), x[:, :, ::-1])
    assert np.array_equal(se.orient_image(x, 2), x[:, ::-1, :])
    assert np.array_equal(se.orient_image(x, 4)[0], [[2, 5, 8], [1, 4, 7], [0, 3, 6]])   # out[r][c] = x[c][N - 1 - r]
    assert np.array_equal(se.orient_image(x, 7), np.rot90(x[:, ::-1, ::-1], axes=(1, 2)))


def test_draw_frequencies():
    B = 4096
    o, nxt = se.draw_orient(se.seeds(B, 20260927))
    assert o.dtype == np.int32 and o.min() >= 0 and o.max() <= 7 and len(set(nxt)) == B
    sd = (B * (1 / 8) * (7 / 8)) ** 0.5
    counts = np.bincount(o, minlength=8)
    assert (np.abs(counts - B / 8) < 5 * sd).all(), counts
    o2, _ = se.draw_orient(nxt)
    assert not np.array_equal(o, o2)


def test_new_symbols_resolve(built):
    L = built.lib()
    for name in NEW:
        assert name in built.EXPORTS and name in built._SIGNATURES and getattr(L, name)
    assert L.gg_version() == 5


def test_entry_points_check_arguments_in_their_documented_order(built):
    L = built.lib()
    p = 16
    for fn in (L.gg_batch_features_oriented, L.gg_batch_features_tracked_oriented):   # (in, orient, out, dtype, B, N, stream)
        assert fn(p, p, p, 4, 4, 9, None) == -1 and fn(p, p, p, -1, 4, 9, None) == -1          # the dtype first
        assert fn(None, None, None, 4, 0, 9, None) == -1
        assert fn(p, p, p, 2, 4, 20, None) == -1 and fn(p, p, p, 2, 4, 1, None) == -1 and fn(p, p, p, 2, -1, 9, None) == -1
        for dt in range(4):
            assert fn(None, None, None, dt, 0, 9, None) == 0                                    # B = 0 before the pointers
        assert fn(None, None, None, 2, 0, 20, None) == -1                                       # ... and after the sizes
        assert fn(None, p, p, 2, 4, 9, None) == -2
        assert fn(p, p, None, 2, 4, 9, None) == -2
        assert fn(p, None, p, 2, 4, 9, None) == -2                                              # orient
        assert fn(p, None, 17, 2, 4, 9, None) == -2                                             # NULL before the alignment of out
        assert fn(p, p, 17, 2, 4, 9, None) == -3
    f = L.gg_batch_symmetry_policy                                                              # (in, orient, out, es, inverse, B, N, stream)
    for es in (0, 3, 8, -1):
        assert f(p, p, p, es, 0, 4, 9, None) == -1
    assert f(p, p, p, 4, 0, 4, 20, None) == -1 and f(p, p, p, 4, 0, 4, 1, None) == -1 and f(p, p, p, 4, 1, -1, 9, None) == -1
    for es in (1, 2, 4):
        assert f(None, None, None, es, 0, 0, 9, None) == 0
    assert f(None, None, None, 4, 0, 0, 20, None) == -1
    assert f(None, p, p, 4, 0, 4, 9, None) == -2 and f(p, None, p, 4, 0, 4, 9, None) == -2 and f(p, p, None, 4, 1, 4, 9, None) == -2
    d = L.gg_batch_draw_orient
    assert d(p, p, -1, None) == -1 and d(None, None, -1, None) == -1
    assert d(None, None, 0, None) == 0
    assert d(None, p, 4, None) == -2 and d(p, None, 4, None) == -2


def test_python_calls_raise_before_a_device_is_touched():
    import torch
    from gymgo_amd import gogame
    st = np.zeros((2, 6, 5, 5), np.uint8)
    tr = torch.zeros((2, 26), dtype=torch.int32)
    for bad in (np.zeros(3, np.int32), np.zeros(2, np.float32), torch.zeros(2), torch.zeros(1, dtype=torch.int64), [0.5, 1.0]):
        with pytest.raises(ValueError):
            gogame.batch_features(st, dtype=torch.uint8, orient=bad)
        with pytest.raises(ValueError):
            gogame.batch_features_tracked(tr, dtype=torch.uint8, orient=bad)
        with pytest.raises(ValueError):
            gogame.batch_symmetry_policy(np.zeros((2, 26), np.float32), bad)
    with pytest.raises(ValueError):
        gogame.batch_features(st, dtype=torch.float64, orient=np.zeros(2, np.int32))
    o2 = np.zeros(2, np.int32)
    for A in (1, 4, 27, 401, 24):                       # not N * N + 1 with N in [2, 19]
        with pytest.raises(ValueError):
            gogame.batch_symmetry_policy(np.zeros((2, A), np.float32), o2)
        with pytest.raises(ValueError):
            gogame.batch_symmetry_policy(torch.zeros((2, A)), o2)
    for bad in (np.zeros((2, 26), np.float64), np.zeros((2, 26), np.int64), torch.zeros((2, 26), dtype=torch.float64),
                torch.zeros((2, 26), dtype=torch.int16), np.zeros(26, np.float32), np.zeros((2, 1, 26), np.float32)):
        with pytest.raises(ValueError):
            gogame.batch_symmetry_policy(bad, o2)
    with pytest.raises(ValueError):
        gogame.batch_symmetry_policy(torch.zeros((2, 26)), o2)                      # a host tensor
    with pytest.raises(ValueError):
        gogame.batch_symmetry_policy(np.zeros((2, 26), np.float32), o2, out=np.zeros((2, 26), np.float32))
    for bad in (np.zeros(4, np.int64), torch.zeros(4, dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int64),
                torch.zeros(8, dtype=torch.int64)[::2]):
        with pytest.raises(ValueError):
            gogame.batch_draw_orient(bad)
    # symmetry needs features
    for call in (lambda: gogame.PuctSearch(st, 2, symmetry=1), lambda: gogame.PuctSearch(st, 2, leaves=2, symmetry=1),
                 lambda: gogame.batch_puct(st, 2, None, symmetry=1), lambda: gogame.puct_play(st, 1, 2, None, symmetry=1),
                 lambda: gogame.puct_actions(st, 2, None, symmetry=1), lambda: gogame.puct(st[0], 2, None, symmetry=1)):
        with pytest.raises(ValueError, match='features'):
            call()


def test_symmetry_none_is_the_search_as_before_and_a_seed_hands_out_views(monkeypatch):
    import torch
    from gymgo_amd import gogame
    monkeypatch.setattr(gogame, '_device', lambda: torch.device('cpu'))
    empty = np.zeros((0, 6, 5, 5), np.uint8)
    with pytest.raises(ValueError, match='features'):
        gogame.puct_selfplay(empty, 1, 2, None, symmetry=1)
    p, v = np.zeros((0, 26), np.float32), np.zeros(0, np.float32)
    for leaves in (None, 3):
        s = gogame.PuctSearch(empty, 2, leaves=leaves, features=torch.float16)
        assert s.orient is None and not hasattr(s, '_sym_rng')
        s = gogame.PuctSearch(empty, 2, leaves=leaves, features=torch.float16, symmetry=5, first_root=3)
        planes, legal = s.select()
        assert tuple(planes.shape) == (0, 16, 5, 5) and tuple(legal.shape) == (0, 26) and legal.dtype == torch.bool
        assert tuple(s.orient.shape) == (0,) and s.orient.dtype == torch.int32
        s.backup(p, v)
        res = gogame.batch_puct(empty, 2, lambda x, l: (p, v), leaves=leaves, features=torch.float16, symmetry=5, first_root=3)
        assert res.visits.shape == (0, 26)
        rec = gogame.puct_selfplay(empty, 0, 2, lambda x, l: (p, v), leaves=leaves, features=torch.float16, symmetry=5)
        assert rec.actions.shape == (0, 0)


def hand_record(as_numpy):
    import torch
    from gymgo_amd import gogame
    R, M, N = 3, 4, 3
    states = np.zeros((R, M, 6, N, N), np.uint8)
    states[:, 1::2, 2] = 1                               # white moves at odd moves ...
    states[2, :, 2] = np.array([1, 0, 1, 0], np.uint8)[:, None, None]      # ... except in game 2, which white starts
    outcome = np.array([1, -1, 0], np.int8)
    lengths = np.array([4, 2, 0], np.int32)
    fields = dict(actions=np.zeros((R, M), np.int64), pi=np.zeros((R, M, N * N + 1), np.float32), value=np.zeros((R, M), np.float32),
                  outcome=outcome, lengths=lengths, final_states=states[:, -1].copy(), states=states)
    if not as_numpy:
        fields = {k: torch.from_numpy(x) for k, x in fields.items()}
    return gogame.SelfPlay(**fields)


@pytest.mark.parametrize('as_numpy', (False, True))
def test_selfplay_targets_on_a_hand_written_record(as_numpy):
    import torch
    from gymgo_amd import gogame
    rec = hand_record(as_numpy)
    games = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2])
    moves = np.array([0, 1, 3, 0, 1, 2, 0, 1, 3])
    z, valid = gogame.selfplay_targets(rec, games, moves)
    assert z.dtype == torch.float32 and valid.dtype == torch.bool
    #           game 0 (black won)   game 1 (white won)   game 2 (running)
    assert z.tolist() == [1.0, -1.0, -1.0, -1.0, 1.0, -1.0, 0.0, 0.0, 0.0]
    assert valid.tolist() == [True, True, True, True, True, False, False, False, False]
    z2, _ = gogame.selfplay_targets(rec, torch.from_numpy(games), torch.from_numpy(moves).to(torch.int32))
    assert torch.equal(z, z2)
    with pytest.raises(ValueError):
        gogame.selfplay_targets(rec._replace(states=None), games, moves)
    with pytest.raises(ValueError):
        gogame.selfplay_batch(rec._replace(states=None), games, moves, np.zeros(9, np.int32))
    with pytest.raises(ValueError):
        gogame.selfplay_batch(rec, games, moves, np.zeros(9, np.int32), dtype=torch.float64)
    with pytest.raises(ValueError):
        gogame.selfplay_batch(rec, games, moves, np.zeros(8, np.int32))
    with pytest.raises(ValueError):
        gogame.selfplay_targets(rec, games, moves[:5])
