"""CPU: what tests/test_gpu_past.py relies on, without a device - the premises of the history planes' definition
(tests/past_expect.py): the move plane occ_t & ~occ_{t+1} is exactly the point played, nothing for a pass; the game set holds
captures of several stones, passes and games longer than the largest ring; the planes turn with the board.  And the binding
table of the past family (_lib.ABI_PAST) against its header (include/gymgo_amd_past.h), as tests/test_host_abi.py holds
_lib.ABI against include/gymgo_amd.h, and the ValueErrors of every new argument, raised before a device is touched."""
import numpy as np
import pytest

import past_expect as pe
import plane_cases as pc


@pytest.mark.parametrize('N', pc.SIZES)
def test_move_plane_is_the_point_played(N):
    """An independent statement of occ_t & ~occ_{t+1}: at every ply the plane has exactly one point, the recorded action's -
    or none, for a pass."""
    P = N * N
    for g, game in enumerate(pe.games(N)):
        assert len(game.states) == len(game.actions) + 1
        for k, a in enumerate(game.actions):
            p = pe.planes(game.states[:k + 2], 2, True)
            assert p.shape == (5, N, N)
            if a == P:
                assert not p[4].any(), (N, g, k)
            else:
                assert p[4].sum() == 1 and p[4].ravel()[a] == 1, (N, g, k)
            # and through a longer window: the move t plies ago, seen from the end of the game so far
            if k + 2 >= 4:
                q = pe.planes(game.states[:k + 2], 4, True)
                for t in range(3):
                    a_t = game.actions[k - t]
                    want = np.zeros(P, np.uint8)
                    if a_t != P:
                        want[a_t] = 1
                    assert np.array_equal(q[8 + t].ravel(), want), (N, g, k, t)


@pytest.mark.parametrize('N', [n for n in pc.SIZES if n >= 3])
def test_game_set_is_not_vacuous(N):
    """A ply that captures at least two stones, a pass, and a game longer than the largest ring used - by the oracle alone."""
    P = N * N
    big_capture = passed = False
    for game in pe.games(N):
        stones = (game.states[:, 0] != 0).sum(axis=(1, 2)) + (game.states[:, 1] != 0).sum(axis=(1, 2))
        for k, a in enumerate(game.actions):
            passed |= a == P
            if a != P and stones[k] + 1 - stones[k + 1] >= 2:
                big_capture = True
    assert big_capture and passed, (N, big_capture, passed)
    assert max(len(g.actions) for g in pe.games(N)) > pe.LARGEST_RING


def test_absent_positions_and_the_view():
    N = 5
    game = pe.games(N)[1]
    seq = game.states[:4]
    p = pe.planes(seq, 8, True)
    assert p.shape == (23, N, N) and not p[8:16].any() and not p[16 + 3:].any()
    white = bool(seq[-1][2, 0, 0])
    for t in range(4):
        s = seq[-1 - t]
        assert np.array_equal(p[2 * t], s[1 if white else 0]) and np.array_equal(p[2 * t + 1], s[0 if white else 1])
    assert np.array_equal(pe.planes(seq, 1, False), p[:2]) and pe.planes(seq, 1, True).shape == (2, N, N)
    # the ring a sequence of pushes leaves, and what a board sees through it
    rows, count = pe.ring(game.states[:7], 3, N)
    assert count == 7 and np.array_equal(rows[0], pe.rows_of(game.states[6])) and np.array_equal(rows[2], pe.rows_of(game.states[5]))
    assert int(pe.rows_of(game.states[6])[0, 2]) == int(sum(1 << c for c in range(N) if game.states[6][0, 2, c]))
    assert len(pe.with_ring(game.states[:8], 7, 3)) == 4 and len(pe.with_ring(game.states[:8], 2, 3)) == 3
    assert len(pe.with_ring(game.states[:8], 0, 3)) == 1


@pytest.mark.parametrize('N', pc.SIZES)
def test_planes_turn_with_the_board(N):
    """turned(planes(seq)) == planes(turned seq) in all eight views: the oriented GPU test may use either."""
    for g, game in enumerate(pe.games(N)):
        k = min(len(game.states), 9 + g)
        seq = game.states[:k]
        for T, moves in ((8, True), (2, False)):
            p = pe.planes(seq, T, moves)
            for o in range(8):
                assert np.array_equal(pe.turned(p, o), pe.planes(pe.turned_seq(seq, o), T, moves)), (N, g, T, moves, o)


# ---------------------------------------------------------------- the past family's header against its binding table
def past_declarations():
    """{function: [(C type without const, is pointer, parameter name)]} of every `int32_t gg_*(...);` of
    include/gymgo_amd_past.h, in header order - tests/test_host_abi.py's reading of include/gymgo_amd.h, of this header."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'gymgo_amd_past.h')).read()
    decls = {}
    for m in re.finditer(r'^\s*(?:int32_t|int)\s+(gg_\w+)\s*\((.*?)\);', hdr, flags=re.M | re.S):
        params = []
        for text in m.group(2).split(','):
            text = ' '.join(text.split())
            if text == 'void':
                continue
            pm = re.fullmatch(r'(?:const )?(\w+) ?(\*?) ?(\w+)', text)
            assert pm, (m.group(1), text)
            params.append((pm.group(1), pm.group(2) == '*', pm.group(3)))
        decls[m.group(1)] = params
    return root, decls


PAST_ENTRY_POINTS = ['gg_past_planes', 'gg_past_push', 'gg_past_push_tracked', 'gg_batch_past', 'gg_batch_past_tracked', 'gg_puct_past']


def test_past_binding_table_matches_its_header(native_built):
    import ctypes
    import os
    import test_host_abi as tha
    from gymgo_amd import _lib
    root, decls = past_declarations()
    assert list(decls) == PAST_ENTRY_POINTS
    assert tha._abi_mismatches(decls, _lib.ABI_PAST) == []
    assert _lib.EXPORTS_PAST == tuple(decls) and not set(decls) & (set(_lib.EXPORTS) | set(_lib.EXPORTS_AREA))
    dropped = dict(_lib.ABI_PAST, gg_batch_past=_lib.ABI_PAST['gg_batch_past'][:3] + _lib.ABI_PAST['gg_batch_past'][4:])
    assert any('12 parameters in the header, 11 in the table' in b for b in tha._abi_mismatches(decls, dropped))    # the comparison can fail
    for f, (argtypes, restype) in _lib._SIGNATURES_PAST.items():
        assert restype is ctypes.c_int32
        assert argtypes == [p.kind if isinstance(p.kind, type) else ctypes.c_void_p for p in _lib.ABI_PAST[f]]
    L = ctypes.CDLL(_lib.LIB_PATH)
    doc = open(os.path.join(root, 'INTEGRATION.md')).read()
    for name in decls:
        assert hasattr(L, name) and name in doc, name
    assert native_built.gg_version() == _lib.ABI_VERSION == 5 and len(_lib.EXPORTS) == 79
    for T in range(-1, 11):
        for moves in (-1, 0, 1, 2):
            want = pe.plane_count(T, moves) if 1 <= T <= 8 and moves in (0, 1) else -1
            assert native_built.gg_past_planes(T, moves) == want, (T, moves)
    assert native_built.gg_past_planes(8, 1) == 23


def test_entry_point_checks_come_before_any_device_work(native_built):
    """The codes and their order, with pointers that are never followed: sizes, then arguments, then the zero-work return,
    then NULL pointers, then alignment."""
    L = native_built
    BADSIZE, BADARG, NULLPTR = -1, -2, -3
    import re, os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gymgo_amd.h')).read()
    codes = {n: int(v) for n, v in re.findall(r'#define\s+(GG_E_\w+)\s+\(?(-?\d+)\)?', hdr)}
    BADSIZE, BADARG, NULLPTR = codes['GG_E_BADSIZE'], codes['GG_E_BADARG'], codes['GG_E_NULLPTR']
    p, odd = 4096, 4098
    # gg_batch_past(states, rows, count, H, T, moves, orient, out, out_dtype, B, N, stream)
    for fn in (L.gg_batch_past, L.gg_batch_past_tracked):
        assert fn(p, p, p, 1, 9, 0, None, p, 3, 1, 1, None) == BADSIZE          # N first, whatever T is
        assert fn(p, p, p, 1, 8, 0, None, p, 4, 1, 9, None) == BADSIZE          # dtype
        assert fn(p, p, p, 1, 8, 0, None, p, 3, -1, 9, None) == BADSIZE
        assert fn(None, p, p, 1, 0, 0, None, p, 3, 1, 9, None) == BADARG        # T before NULL
        assert fn(None, p, p, 1, 9, 0, None, p, 3, 0, 9, None) == BADARG        # ... and before the zero-work return
        assert fn(None, p, p, 1, 8, 2, None, p, 3, 1, 9, None) == BADARG
        assert fn(None, p, p, 0, 8, 1, None, p, 3, 1, 9, None) == BADARG        # H < 1 with a ring
        assert fn(None, None, None, 0, 8, 1, None, None, 3, 0, 9, None) == 0    # B == 0 before NULL; H is not looked at without a ring
        assert fn(None, None, None, 0, 8, 1, None, p, 3, 1, 9, None) == NULLPTR
        assert fn(p, p, None, 1, 8, 1, None, p, 3, 1, 9, None) == NULLPTR       # one of the pair alone
        assert fn(p, None, p, 1, 8, 1, None, p, 3, 1, 9, None) == NULLPTR
        assert fn(p, p, p, 1, 8, 1, None, None, 3, 1, 9, None) == NULLPTR
        assert fn(p, odd, p, 1, 8, 1, None, p, 3, 1, 9, None) == BADARG         # alignment last
        assert fn(p, p, p, 1, 8, 1, odd, p, 3, 1, 9, None) == BADARG
        assert fn(p, p, p, 1, 8, 1, None, odd, 0, 1, 9, None) == BADARG         # out to its element
    assert L.gg_batch_past_tracked(odd, p, p, 1, 8, 1, None, p, 3, 1, 9, None) == BADARG
    # gg_past_push(states, mask, rows, count, H, B, N, stream)
    for fn in (L.gg_past_push, L.gg_past_push_tracked):
        assert fn(p, None, p, p, 1, 1, 20, None) == BADSIZE
        assert fn(None, None, p, p, 0, 1, 9, None) == BADARG
        assert fn(None, None, None, None, 1, 0, 9, None) == 0
        assert fn(None, None, p, p, 1, 1, 9, None) == NULLPTR
        assert fn(p, None, None, p, 1, 1, 9, None) == NULLPTR and fn(p, None, p, None, 1, 1, 9, None) == NULLPTR
        assert fn(p, None, odd, p, 1, 1, 9, None) == BADARG and fn(p, None, p, odd, 1, 1, 9, None) == BADARG
    # gg_puct_past(R, N, C, L, boards, links, rows, count, H, T, moves, leaf, leaf_id, orient, out, out_dtype, stream)
    f = L.gg_puct_past
    assert f(1, 1, 4, 1, p, p, p, p, 1, 8, 1, p, p, None, p, 3, None) == BADSIZE
    assert f(1, 9, 4, 1, p, p, p, p, 1, 8, 1, p, p, None, p, 7, None) == BADSIZE
    assert f(1, 9, 0, 1, None, p, p, p, 1, 8, 1, p, p, None, p, 3, None) == BADARG
    assert f(1, 9, 4, 5, None, p, p, p, 1, 8, 1, p, p, None, p, 3, None) == BADARG
    assert f(1, 9, 4, 0, None, p, p, p, 1, 8, 1, p, p, None, p, 3, None) == BADARG
    assert f(1, 9, 2 ** 31 - 1, 1, None, p, p, p, 1, 8, 1, p, p, None, p, 3, None) == BADARG
    assert f(0, 9, 4, 1, None, p, p, p, 1, 9, 1, p, p, None, p, 3, None) == BADARG
    assert f(0, 9, 4, 1, None, None, None, None, 0, 8, 1, None, None, None, None, 3, None) == 0
    for hole in (4, 5, 11, 12, 14):
        args = [1, 9, 4, 1, p, p, p, p, 1, 8, 1, p, p, None, p, 3, None]
        args[hole] = None
        assert f(*args) == NULLPTR, hole
    assert f(1, 9, 4, 1, p, p, p, None, 1, 8, 1, p, p, None, p, 3, None) == NULLPTR
    for hole in (4, 5, 6, 7, 11, 12, 13):
        args = [1, 9, 4, 1, p, p, p, p, 1, 8, 1, p, p, None, p, 3, None]
        args[hole] = odd
        assert f(*args) == BADARG, hole
    assert f(1, 9, 4, 1, p, p, p, p, 1, 8, 1, p, p, None, 4097, 2, None) == BADARG           # out to its element


def test_value_errors_before_a_device_is_touched(native_built):
    """Every new argument's ValueError, on a box without a device: none of these calls gets as far as one."""
    import torch
    from gymgo_amd import gogame
    assert gogame.PAST_MAX_POSITIONS == 8
    SH = gogame.StoneHistory
    cpu = torch.device('cpu')    # (tensors of the history object only: no launch is reached)
    for kw in (dict(positions=0), dict(positions=9), dict(positions=2.0), dict(positions=True), dict(moves=2), dict(moves='yes'),
               dict(positions=4, capacity=2), dict(capacity=0), dict(capacity=1.5)):
        with pytest.raises(ValueError):
            SH(3, 5, device=cpu, **kw)
    for B, N in ((-1, 5), (3, 1), (3, 20)):
        with pytest.raises(ValueError):
            SH(B, N, device=cpu)
    h = SH(3, 5, positions=4, moves=True, device=cpu)
    assert (h.positions, h.moves, h.capacity, h.planes) == (4, True, 3, 11)
    assert tuple(h.rows.shape) == (3, 3, 2, 5) and h.rows.dtype == torch.int32 and tuple(h.count.shape) == (3,)
    assert SH(2, 9, positions=1, device=cpu).capacity == 1 and SH(2, 9, positions=8, capacity=12, device=cpu).capacity == 12
    assert gogame.past_plane_count(8, True) == 23 and gogame.past_plane_count(3) == 6
    states = np.zeros((3, 6, 5, 5), np.uint8)
    with pytest.raises(ValueError):
        h.push(np.zeros((2, 6, 5, 5), np.uint8))
    with pytest.raises(ValueError):
        h.push(np.zeros((3, 6, 4, 4), np.uint8))
    with pytest.raises(ValueError):
        h.push(states, mask=np.ones(2, bool))
    with pytest.raises(ValueError):
        h.push(states, mask=np.ones(3, np.int64))
    with pytest.raises(ValueError):
        h.push_tracked(torch.zeros((3, 27), dtype=torch.int32))
    with pytest.raises(ValueError):
        h.push_tracked(torch.zeros((2, 26), dtype=torch.int32))
    with pytest.raises(ValueError):
        h.reset(mask=np.ones(4, bool))
    assert h.reset(np.array([True, False, True])) is h and h.reset() is h
    for bad in (dict(dtype=torch.int32), dict(orient=np.zeros(2, np.int64)), dict(orient=np.zeros(3)),
                dict(out=torch.zeros((3, 11, 5, 5), dtype=torch.uint8))):
        with pytest.raises(ValueError):
            gogame.batch_past_planes(states, h, **bad)
    with pytest.raises(ValueError):
        gogame.batch_past_planes(states, None)
    with pytest.raises(ValueError):
        gogame.batch_past_planes(states[:2], h)
    with pytest.raises(ValueError):
        gogame.batch_past_planes(np.zeros((3, 6, 4, 4), np.uint8), h)
    with pytest.raises(ValueError):
        gogame.batch_past_planes(states, h, dtype=torch.bfloat16)      # NumPy has no bfloat16
    with pytest.raises(ValueError):
        gogame.batch_past_planes_tracked(torch.zeros((3, 27), dtype=torch.int32), h)
    with pytest.raises(ValueError):
        gogame.batch_past_planes_tracked(torch.zeros((3, 26), dtype=torch.int32), SH(2, 5, device=cpu))
    for kw in (dict(positions=0), dict(positions=9), dict(moves=3), dict(dtype=torch.int8)):
        with pytest.raises(ValueError):
            gogame.past_planes(states, **kw)
    with pytest.raises(ValueError):
        gogame.past_planes(states[0])
    # the search and its loops: past= needs features=, and must be what it says
    ev = lambda *a: None
    with pytest.raises(ValueError, match='features'):
        gogame.PuctSearch(states, 4, past=h)
    for fn in (gogame.batch_puct, gogame.puct_actions):
        with pytest.raises(ValueError, match='features'):
            fn(states, 4, ev, past=h)
    with pytest.raises(ValueError, match='features'):
        gogame.puct(states[0], 4, ev, past=h)
    with pytest.raises(ValueError, match='features'):
        gogame.puct_play(states, 2, 4, ev, past=8)
    with pytest.raises(ValueError, match='features'):
        gogame.puct_selfplay(states, 2, 4, ev, past=(8, True))
    f16 = torch.float16
    with pytest.raises(ValueError):
        gogame.PuctSearch(states, 4, features=f16, past=8)                     # a StoneHistory, not a request
    with pytest.raises(ValueError):
        gogame.PuctSearch(states, 4, features=f16, past=SH(2, 5, device=cpu))  # of R boards
    with pytest.raises(ValueError):
        gogame.PuctSearch(states, 4, features=f16, past=SH(3, 9, device=cpu))  # of size N
    for bad in (0, 9, (8, 2), (8, True, 1), 'eight', 2.0, True, [8, True]):
        with pytest.raises(ValueError):
            gogame.puct_play(states, 2, 4, ev, features=f16, past=bad)
        with pytest.raises(ValueError):
            gogame.puct_selfplay(states, 2, 4, ev, features=f16, past=bad)
    rec = gogame.SelfPlay(None, None, None, None, None, None, None)
    with pytest.raises(ValueError):
        gogame.selfplay_batch(rec, [0], [0], [0], past=(8, True))              # no states in the record
