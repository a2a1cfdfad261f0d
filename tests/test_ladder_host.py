"""CPU: the ladder planes (gogame.batch_ladder / batch_ladder_tracked, gg_batch_ladder*) without a device - the expectation
module (ladder_expect) on hand-worked positions with the expected points written out, each with either colour to move and
with the colours swapped; the bounds; and the argument checks of the C entry points and the Python API."""
import numpy as np
import pytest

import features_expect as fe
import ladder_expect as le


@pytest.fixture(scope='module')
def built(native_built):
    from gymgo_amd import _lib
    return _lib


def plane(N, pts):
    g = np.zeros((N, N), np.uint8)
    for p in pts:
        g[p] = 1
    return g


def check(rows, x_lad=(), o_lad=(), x_cap=(), o_cap=(), x_esc=(), o_esc=(), aborted=0, **kw):
    """The position `rows` (black = X) in all four forms.  x_lad / o_lad: the laddered stones of X / O; x_cap / o_cap: the
    ladder captures X / O has (plane 2 when that colour moves); x_esc / o_esc: the ladder escapes X / O has (plane 3 when that
    colour moves).  -> the stats of the first form."""
    N = len(rows)
    first = None
    for swapped in (False, True):
        for white_to_move in (False, True):
            s = fe.board(le.swap(rows) if swapped else rows, white_to_move=white_to_move, **kw)
            got, ab, st = le.ladder(s, stats=True)
            first = first or st
            assert got.shape == (4, N, N) and got.dtype == np.uint8
            x_moves = swapped == white_to_move         # X is black unless swapped; own is black unless white moves
            want = [x_lad, o_lad, x_cap, x_esc] if x_moves else [o_lad, x_lad, o_cap, o_esc]
            for p in range(4):
                assert np.array_equal(got[p], plane(N, want[p])), (rows, swapped, white_to_move, le.NAMES[p], got[p], want[p])
            assert ab == aborted
    return first


def test_textbook_ladder_runs_to_the_edge_and_a_breaker_stops_it():
    assert le.LADDER9 == ['.X.......', 'XO.......', 'X........'] + ['.........'] * 6
    # the white stone is caught by the atari at (1, 2); the black stone (0, 1) on the edge, with two liberties, by the one at
    # (0, 2) - the atari at (0, 0) is answered at (0, 2) with three liberties
    st = check(le.LADDER9, x_lad=[(0, 1)], o_lad=[(1, 1)], x_cap=[(1, 2)], o_cap=[(0, 2)])
    assert st['queries'] == 4 and st['depth'] > 6 and st['aborts'] == 0
    # the breaker on the path: the white stone gets away, the planes about it are empty
    st = check(le.BROKEN9, x_lad=[(0, 1)], o_cap=[(0, 2)])
    assert st['free'] == 1


def test_only_the_atari_that_works_is_marked():
    # of the two ataris on (1, 1) only (1, 2) works: after (2, 1) white extends to (1, 2) and has (0, 2), (1, 3), (2, 2)
    got, ab = le.ladder(fe.board(le.LADDER9))
    assert got[2].sum() == 1 and got[2][1, 2] == 1 and got[2][2, 1] == 0 and ab == 0


def test_a_prey_in_atari_that_lives_only_by_capturing_a_chaser():
    # white (0, 2), (1, 2): the extension (0, 1) leaves one liberty, the capture at (2, 3) three.  The black pair in atari
    # gets out at (2, 3) itself and by capturing the white pair at (0, 1)
    check(le.CAPTURE_SAVES, o_esc=[(2, 3)], x_esc=[(0, 1), (2, 3)])


def test_an_extension_that_is_suicide_escapes_nothing():
    check(le.SUICIDE, o_lad=[(0, 1), (1, 1)])


def test_ko_inside_the_ladder_and_root_ko():
    # white (2, 2) captures (1, 2) at (1, 1): two liberties, and the attacker cannot take back at (1, 2), the ko point, so
    # white connects out; black (1, 2) gets out at (1, 1) and by capturing (2, 2) at (3, 2)
    check(le.KO, o_esc=[(1, 1)], x_esc=[(1, 1), (3, 2)])
    st = le.ladder(fe.board(le.KO, white_to_move=True), stats=True)[2]
    assert st['depth'] == 2 and st['nodes'] == 3      # A after the capture, D after the one atari that is legal; D for black's capture
    # (1, 1) as the ROOT ko point: white to move cannot capture there and is laddered ...
    s = fe.board(le.KO, white_to_move=True, invalid=[(1, 1)])
    assert fe.features(s)[11][1, 1] == 1
    got, ab = le.ladder(s)
    assert np.array_equal(got[0], plane(7, [(2, 2)])) and not got[1:].any()
    # ... and for the other side's query it does not apply: black (1, 2), the defender that is not to move, still gets out,
    # so it is in no plane; with black to move the mark is no ko point (no white chain in atari next to it) and nothing changes
    s = fe.board(le.KO, invalid=[(1, 1)])
    assert not fe.features(s)[11].any()
    got, ab = le.ladder(s)
    assert np.array_equal(got[3], plane(7, [(1, 1), (3, 2)])) and not got[:3].any()


def test_corner_to_corner_ladder_at_19_stays_inside_both_bounds():
    st = check(le.LADDER19, x_lad=[(0, 1)], o_lad=[(1, 1)], x_cap=[(1, 2)], o_cap=[(0, 2)])
    assert 3 * 19 < st['depth'] < le.max_depth(19) and st['nodes'] < le.max_nodes(19) and st['aborts'] == 0


def bound_hits(state):
    """Which bound each aborted query of the state ran into, in the order of the queries."""
    N = state.shape[-1]
    hits = []
    enter = le.Budget.enter

    def spy(self, depth):
        if depth > le.max_depth(N):
            hits.append('depth')
        elif self.nodes + 1 > le.max_nodes(N):
            hits.append('nodes')
        return enter(self, depth)

    le.Budget.enter = spy
    try:
        le.ladder(state)
    finally:
        le.Budget.enter = enter
    return hits


class far_bounds:
    """The expectation with both bounds out of reach (of these boards: 300 plies, 20 000 nodes)."""

    def __enter__(self):
        self.saved = le.max_depth, le.max_nodes
        le.max_depth, le.max_nodes = (lambda N: 300), (lambda N: 20000)

    def __exit__(self, *exc):
        le.max_depth, le.max_nodes = self.saved


def test_the_searched_bound_boards_abort_one_query_on_the_bound_they_are_named_for():
    for rows, why in ((le.NODE_BOUND7, 'nodes'), (le.NODE_BOUND9, 'nodes'), (le.DEPTH_BOUND7, 'depth'),
                      (le.ABORT_DEPTH_ATTACKER, 'depth'), (le.ABORT_DEPTH_DEFENDER, 'depth'),
                      (le.ABORT_NODES_ATTACKER, 'nodes'), (le.ABORT_NODES_DEFENDER, 'nodes')):
        for s in le.forms(rows):
            got, ab, st = le.ladder(s, stats=True)
            assert bound_hits(s) == [why] and ab == 1 and st['aborts'] == 1, (rows, why)
    # on the three older boards the answer found so far and the conservative one are the same: the planes, written out,
    # are those of the search without bounds
    for rows, want in ((le.NODE_BOUND7, dict(o_lad=[(1, 1)], x_cap=[(2, 1)], x_esc=[(3, 3), (4, 1)], o_esc=[(3, 3), (4, 1), (5, 1)])),
                       (le.DEPTH_BOUND7, dict(x_lad=[(0, 6), (1, 3)], o_lad=[(5, 5)], x_cap=[(5, 4)], o_cap=[(1, 6), (2, 3)]))):
        check(rows, aborted=1, **want)
        with far_bounds():
            check(rows, aborted=0, **want)


def test_aborted_attacker_queries_answer_not_captured():
    # DEPTH: white's atari at (0, 1) on black (0, 0) works, 33 plies deep; at 4 N = 28 it is aborted and not marked, and
    # black (0, 0) is laddered all the same, by the atari at (1, 0)
    st = check(le.ABORT_DEPTH_ATTACKER, aborted=1, x_lad=[(0, 0)], o_cap=[(1, 0)])
    assert st['depth'] == le.max_depth(7) and st['queries'] == 2
    with far_bounds():
        st = check(le.ABORT_DEPTH_ATTACKER, aborted=0, x_lad=[(0, 0)], o_cap=[(0, 1), (1, 0)])
        assert st['depth'] == 33
    # NODES: black's atari at (5, 4) on white (6, 4) works after more than 16 N = 112 nodes; aborted it is not marked, and
    # with the other atari failing white (6, 4) is not laddered
    common = dict(x_esc=[(5, 5)], o_esc=[(3, 6), (5, 5)])
    st = check(le.ABORT_NODES_ATTACKER, aborted=1, **common)
    assert st['depth'] < le.max_depth(7)
    with far_bounds():
        check(le.ABORT_NODES_ATTACKER, aborted=0, o_lad=[(6, 4)], x_cap=[(5, 4)], **common)


def test_aborted_defender_queries_answer_escapes():
    # DEPTH: black (0, 0) in atari does not get out at (1, 0); aborted at 4 N plies the extension is marked as an escape and
    # the stone is not laddered
    check(le.ABORT_DEPTH_DEFENDER, aborted=1, x_esc=[(1, 0)])
    with far_bounds():
        check(le.ABORT_DEPTH_DEFENDER, aborted=0, x_lad=[(0, 0)])
    # NODES: white (0, 2) in atari gets out neither by extending to (0, 3) nor by capturing at (1, 0) (the mark there is the
    # escape of white (1, 1)); the query of (0, 3) needs more than 16 N nodes: aborted it is an escape, for white to move,
    # and (0, 2) is not laddered
    common = dict(x_esc=[(0, 3), (1, 0)])
    check(le.ABORT_NODES_DEFENDER, aborted=1, o_lad=[(4, 6)], o_esc=[(0, 3), (1, 0)], **common)
    with far_bounds():
        check(le.ABORT_NODES_DEFENDER, aborted=0, o_lad=[(0, 2), (4, 6)], o_esc=[(1, 0)], **common)


def test_empty_full_small_and_ended_boards():
    check(['.....'] * 5)
    check(['XXXXX'] * 5)
    check(['XOXOX'] * 5)
    check(['..', '..'])
    check(['XX', 'XX'])
    # a hand-made chain without a liberty is never asked about and stays: the white stones' shared liberty is suicide
    check(['XO', 'O.'], o_lad=[(0, 1), (1, 0)])
    check(['X.', '.O'], x_lad=[(0, 0)], o_lad=[(1, 1)], x_cap=[(0, 1), (1, 0)], o_cap=[(0, 1), (1, 0)])
    # an ended game keeps planes 0 and 1 and loses 2 and 3
    s = fe.board(le.LADDER9, done=True)
    got, ab = le.ladder(s)
    live, _ = le.ladder(fe.board(le.LADDER9))
    assert np.array_equal(got[:2], live[:2]) and live[2].any() and not got[2:].any()


def test_orientation_is_the_planes_of_the_turned_position():
    import symmetry_expect as se
    s = np.stack([fe.board(le.LADDER9)] * 8)
    got, ab = le.oriented(s, np.arange(8))
    plain, _ = le.batch_ladder(s)
    turned = se.orient_images(plain, np.arange(8))
    for k in range(8):
        one, a = le.ladder(se.orient_image(s[0], k))
        assert np.array_equal(got[k], one) and ab[k] == a
        if not a:     # without an aborted query the planes are geometric; with one the view's own row-major order decides
            assert np.array_equal(got[k], turned[k]), k
    assert (ab == 0).sum() >= 4 and ab[0] == 0


def test_entry_points_check_arguments_without_device(built):
    L = built.lib()
    for name in ('gg_batch_ladder', 'gg_batch_ladder_tracked'):
        assert name in built.EXPORTS and name in built._SIGNATURES and getattr(L, name)
    p = 16
    for fn in (L.gg_batch_ladder, L.gg_batch_ladder_tracked):
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
    assert gogame.LADDER_PLANES == 4 and gogame.LADDER_NAMES == le.NAMES
    st = np.zeros((2, 6, 5, 5), np.uint8)
    tr = torch.zeros((2, 26), dtype=torch.int32)
    for bad in (torch.float64, torch.int8, torch.bool, np.float16, 'float16', None):
        with pytest.raises(ValueError):
            gogame.batch_ladder(st, dtype=bad)
        with pytest.raises(ValueError):
            gogame.ladder(st[0], dtype=bad)
        with pytest.raises(ValueError):
            gogame.batch_ladder_tracked(tr, dtype=bad)
    for out in (torch.zeros((2, 4, 5, 5), dtype=torch.float16), torch.zeros((2, 4, 5, 4), dtype=torch.float16), np.zeros((2, 4, 5, 5)),
                torch.zeros((2, 4, 5, 5), dtype=torch.float32)):
        with pytest.raises(ValueError):
            gogame.batch_ladder(st, dtype=torch.float16, out=out)
        with pytest.raises(ValueError):
            gogame.batch_ladder_tracked(tr, dtype=torch.float16, out=out)
    with pytest.raises(ValueError):
        gogame.batch_ladder(np.zeros((2, 5, 5, 5), np.uint8))
    with pytest.raises(ValueError):
        gogame.batch_ladder(st, dtype=torch.bfloat16)              # NumPy in, NumPy out: there is no NumPy bfloat16
    with pytest.raises(ValueError):
        gogame.ladder(st[0], dtype=torch.bfloat16)
    for orient in ([0, 1, 2], np.zeros(2, np.float32), torch.zeros(2, dtype=torch.bool)):
        with pytest.raises(ValueError):
            gogame.batch_ladder(st, orient=orient)
        with pytest.raises(ValueError):
            gogame.batch_ladder_tracked(tr, orient=orient)
    with pytest.raises(ValueError):
        gogame.batch_ladder_tracked(torch.zeros((2, 27), dtype=torch.int32))


def test_ladder_has_no_cpu_fallback(built):
    import torch
    from gymgo_amd import gogame
    if torch.cuda.is_available():
        pytest.skip('device present')
    st = np.zeros((2, 6, 9, 9), np.uint8)
    for call in (lambda: gogame.batch_ladder(st), lambda: gogame.ladder(st[0]),
                 lambda: gogame.batch_ladder_tracked(torch.zeros((2, 46), dtype=torch.int32))):
        with pytest.raises(built.GymGoNativeError):
            call()


def test_ladder_needs_features(monkeypatch):
    import torch
    from gymgo_amd import gogame
    monkeypatch.setattr(gogame, '_device', lambda: torch.device('cpu'))
    empty = np.zeros((0, 6, 5, 5), np.uint8)
    p, v = np.zeros((0, 26), np.float32), np.zeros(0, np.float32)
    ev3 = lambda planes, legal, ladder: (p, v)
    for call in (lambda: gogame.PuctSearch(empty, 2, ladder=True),
                 lambda: gogame.batch_puct(empty, 2, ev3, ladder=True),
                 lambda: gogame.puct_actions(empty, 2, ev3, ladder=True),
                 lambda: gogame.puct(np.zeros((6, 5, 5), np.uint8), 2, ev3, ladder=True),
                 lambda: gogame.puct_play(empty, 1, 2, ev3, ladder=True),
                 lambda: gogame.puct_selfplay(empty, 1, 2, ev3, ladder=True)):
        with pytest.raises(ValueError, match='features'):
            call()


def test_ladder_on_no_roots_hands_out_empty_planes(monkeypatch):
    import torch
    from gymgo_amd import gogame
    monkeypatch.setattr(gogame, '_device', lambda: torch.device('cpu'))
    empty = np.zeros((0, 6, 5, 5), np.uint8)
    A = 26
    p, v = np.zeros((0, A), np.float32), np.zeros(0, np.float32)
    for leaves in (None, 3):
        for life in (False, True):
            s = gogame.PuctSearch(empty, 2, leaves=leaves, features=torch.bfloat16, symmetry=5, life=life, ladder=True)
            res = s.select()
            assert len(res) == 3 + life and tuple(res[-1].shape) == (0, 4, 5, 5) and res[-1].dtype == torch.bfloat16
            s.backup(p, v)
        assert len(gogame.PuctSearch(empty, 2, leaves=leaves, features=torch.float16).select()) == 2     # ladder=False: as ever
        seen = []

        def ev(x, l, life, ladder):
            seen.append((tuple(life.shape), tuple(ladder.shape), ladder.dtype))
            return p, v

        gogame.batch_puct(empty, 3, ev, leaves=leaves, features=torch.float16, life=True, ladder=True)
        assert seen == [((0, 4, 5, 5), (0, 4, 5, 5), torch.float16)] * 3
        ev3 = lambda x, l, ladder: (p, v)
        assert gogame.puct_selfplay(empty, 0, 2, ev3, leaves=leaves, features=torch.float16, ladder=True).actions.shape == (0, 0)
        assert gogame.puct_play(empty, 2, 2, ev3, leaves=leaves, features=torch.float16, ladder=True)[0].shape == (0, 2)


def test_documents_name_the_ladder_entry_points():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'INTEGRATION.md')).read()
    for name in ('gg_batch_ladder', 'gg_batch_ladder_tracked'):
        assert name in text, name
