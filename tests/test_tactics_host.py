"""CPU: the `tactical` playout policy without a device - the rule (mc_tactics_expect.tiers) on hand-made positions point by
point, the properties of the ply-by-ply expectation (mc_tactics_expect.tactical_rollout) that the GPU tests compare against,
the binding table of the family (_lib.ABI_TACTICS) against its header, and the argument checks of the Python API and the C
entry points."""
import os

import numpy as np
import pytest

import features_expect as fe
import mc_expect as mc
import mc_policy_expect as mp
import mc_tactics_expect as mt
from oracle import c_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built(native_built):
    from gymgo_amd import _lib
    return _lib


def test_tiers_on_hand_made_positions_point_by_point():
    pos = mt.crafted_positions()
    names = [p[0] for p in pos]
    for want in ('capture_centre', 'capture_edge', 'capture_corner', 'capture_two_groups', 'escape_one_empty', 'escape_two_empty',
                 'escape_is_capture', 'ko_point_not_in_C', 'capture_centre_white', 'escape_two_empty_white'):
        assert want in names
    for name, b, C, E in pos:
        N = b.shape[-1]
        counts = np.stack([fe.group_liberties(b)]).astype(np.int32)         # low from features_expect's per-group count ...
        gc, ge, gf = mt.tiers(b[None], counts)
        gc2, ge2, gf2 = mt.tiers(b[None])                                   # ... and from the batched one
        assert np.array_equal(gc, gc2) and np.array_equal(ge, ge2) and np.array_equal(gf, gf2), name
        for y in range(N):
            for x in range(N):
                assert bool(gc[0, y, x]) == bool(C[y, x]), (name, 'C', y, x)
                assert bool(ge[0, y, x]) == bool(E[y, x]), (name, 'E', y, x)
        assert np.array_equal(gf[0], mp.candidates(b[None])[0].reshape(N, N)), name
        assert not (gc[0] & mp.eyes(b[None])[0]).any() and not (ge[0] & mp.eyes(b[None])[0]).any(), name
    by = {p[0]: p for p in pos}
    # several groups at once: the move at the one capture point takes two stones of two groups
    b = by['capture_two_groups'][1]
    nxt = c_oracle.next_state(b, 2 * 5 + 2)
    assert int(b[1].sum()) - int(nxt[1].sum()) == 2
    # the ko point: the black stone next to it IS in atari and the point is its last liberty, yet it is not valid
    ko = by['ko_point_not_in_C'][1]
    assert fe.group_liberties(ko)[1, 2] == 1 and ko[0, 1, 2] == 1 and ko[3, 1, 1] == 1 and ko[2].all()
    # a game that has ended has no points in any set
    e = by['capture_centre'][1].copy()
    e[5] = 1
    assert not any(s.any() for s in mt.tiers(e[None]))
    # the seam roots hold what they promise (asserted inside)
    assert mt.seam_roots().shape == (2, 6, 19, 19)


def test_batched_liberty_counts_equal_the_per_board_ones():
    for N in (2, 5, 9, 13):
        roots = mc.make_roots(N, 24, 3 + N, max_ply=2 * N * N, step=max(2, N * N // 12))
        got = mt.group_liberty_counts(roots)
        for i in range(len(roots)):
            assert np.array_equal(np.minimum(got[i], 255), fe.group_liberties(roots[i])), (N, i)


def _chain(board, y, x):
    """(stones, liberties) of the chain of the stone at (y, x) of a board [6, N, N], as sets of points."""
    N = board.shape[-1]
    c = 0 if board[0, y, x] else 1
    assert board[c, y, x]
    seen, todo, libs = {(y, x)}, [(y, x)], set()
    while todo:
        p = todo.pop()
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            q = (p[0] + dy, p[1] + dx)
            if not (0 <= q[0] < N and 0 <= q[1] < N):
                continue
            if board[c][q]:
                if q not in seen:
                    seen.add(q)
                    todo.append(q)
            elif not board[1 - c][q]:
                libs.add(q)
    return seen, libs


def _check_trace(trace, N):
    for live, before, n, act, which, gate, hasC in trace:
        C, E, F = mt.tiers(before)
        eyes = mp.eyes(before)
        assert not (C & eyes).any() and not (E & eyes).any()                     # C and E never meet the eyes
        pt = act < N * N
        assert np.array_equal(~pt, n == 0)                                       # a pass happens only with n = 0
        assert not (~pt & (which != mt.SET_F)).any()                             # ... which only F can have
        nxt, status = c_oracle.batch_next_states(before, act)
        assert not status.any()
        for i in np.flatnonzero(pt & (which != mt.SET_F)):
            b, a = before[i], int(act[i])
            y, x = divmod(a, N)
            white = int(b[2, 0, 0] != 0)
            if which[i] == mt.SET_C:                                              # a move from C lowers the opponent's stone count
                assert gate[i] and C[i, y, x]
                assert int(nxt[i][1 - white].sum()) < int(b[1 - white].sum())
            else:                                                                 # a move from E: the chain it makes has >= 2
                assert gate[i] and not hasC[i] and E[i, y, x]                     # liberties and it touches a chain that had one
                assert len(_chain(nxt[i], y, x)[1]) >= 2
                touched = [(y + dy, x + dx) for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1))
                           if 0 <= y + dy < N and 0 <= x + dx < N and b[white, y + dy, x + dx]]
                assert any(len(_chain(b, *q)[1]) == 1 for q in touched)


def test_tactical_rollout_properties_9x9_and_the_recorded_counts():
    N, B = 9, 64
    st = np.zeros((B, 6, N, N), np.uint8)
    rng0 = c_oracle.rng_seed(1, B)
    trace = []
    fin, rng1, last, steps = mt.tactical_rollout(st, rng0, 8 * N * N, auto_reset=False, trace=trace)
    _check_trace(trace, N)
    assert np.array_equal(mc.plies_from_rng(rng0, rng1), steps)              # the generator advanced by plies * c
    assert (fin[:, 5, 0, 0] == 1).all() and steps.max() < 8 * N * N          # every game ended (by two passes)
    assert (last == N * N).all()
    b, w = c_oracle.batch_areas(fin)
    assert np.array_equal(np.asarray(b) + np.asarray(w), np.full(B, N * N))  # no point is neutral
    got = mt.trace_counts(trace)
    # recorded on the CPU: 1 269 plies from C, 99 from E, 410 closed-gate plies with C not empty, of 6 737; longest game 142
    assert got['C'] >= 500 and got['E'] >= 50 and got['closed_with_C'] >= 100, got
    assert got['C'] + got['E'] + got['F'] == got['plies'] == int(steps.sum())


@pytest.mark.parametrize('N', [2, 3, 4, 5, 6, 7, 13])
def test_tactical_games_end_at_every_size(N):
    B = 16
    st = np.zeros((B, 6, N, N), np.uint8)
    rng0 = c_oracle.rng_seed(1, B)
    trace = []
    fin, rng1, last, steps = mt.tactical_rollout(st, rng0, 8 * N * N, auto_reset=False, trace=trace)
    if N <= 5:
        _check_trace(trace, N)
    assert (fin[:, 5, 0, 0] == 1).all() and steps.max() < 8 * N * N, (N, int(steps.max()))
    assert np.array_equal(mc.plies_from_rng(rng0, rng1), steps)
    got = mt.trace_counts(trace)
    if N == 2:
        assert got['E'] == 0      # (no point of a 2x2 board has two empty neighbours next to a stone in atari that it saves)
    else:
        assert got['C'] > 0


def test_tactical_games_end_on_19x19():
    N, B = 19, 6
    rng0 = c_oracle.rng_seed(1, B)
    fin, rng1, last, steps = mt.tactical_rollout(np.zeros((B, 6, N, N), np.uint8), rng0, 8 * N * N, auto_reset=False)
    assert (fin[:, 5, 0, 0] == 1).all() and steps.max() < 8 * N * N, int(steps.max())   # (recorded: longest game 516 plies)
    assert np.array_equal(mc.plies_from_rng(rng0, rng1), steps)


def test_tactical_rollout_auto_reset_and_frozen_boards():
    N = 5
    roots = np.concatenate([mc.crafted_roots(N), mp.forced_pass_roots(N)])
    rng0 = c_oracle.rng_seed(3, len(roots))
    fin, rng1, last, steps = mt.tactical_rollout(roots, rng0, 40, auto_reset=False)
    assert steps[3] == 0 and last[3] == -1 and rng1[3] == rng0[3] and np.array_equal(fin[3], roots[3])   # the finished game
    assert steps[4] == 2 and last[4] == N * N                                                           # pass, pass
    fin2, rng2, last2, steps2 = mt.tactical_rollout(roots, rng0, 40, auto_reset=True)
    assert (steps2 == 40).all() and np.array_equal(mc.plies_from_rng(rng0, rng2), steps2)
    # ... and the policy is not no_eye_fill
    fin3, _, _, _ = mp.policy_rollout(roots, rng0, 40, auto_reset=True)
    assert not np.array_equal(fin2, fin3)


def test_expected_tactical_results_are_consistent():
    N, R, K = 5, 6, 4
    roots = mc.make_roots(N, R, 9, max_ply=24, step=4)
    full = mt.expected_playouts_tactical(roots, K, 8 * N * N, with_ownership=True)
    assert np.array_equal(full['black_wins'] + full['white_wins'] + full['draws'], np.full(R, K))
    assert full['plies_sum'][-1] == 0
    a = mt.expected_playouts_tactical(roots[:2], K, 8 * N * N, first_root=0)
    b = mt.expected_playouts_tactical(roots[2:], K, 8 * N * N, first_root=2)
    for k in ('black_wins', 'margin_sum', 'plies_sum'):
        assert np.array_equal(np.concatenate([a[k], b[k]]), full[k])
    mv = mt.expected_move_playouts_tactical(roots[:2], 2, 8 * N * N)
    assert np.array_equal(mv['legal'], mc.legal_mask(roots[:2]))
    u = mt.expected_uct_tactical(roots[:2], 3, 2)
    assert (u['root_visits'] == 6).all()


# ---------------------------------------------------------------- the family's header against its binding table
def tactics_declarations():
    """{function: [(C type without const, is pointer, parameter name)]} of every `int32_t gg_*(...);` of
    include/gymgo_amd_tactics.h, in header order - tests/test_host_abi.py's reading of include/gymgo_amd.h, of this header."""
    import re
    hdr = open(os.path.join(ROOT, 'include', 'gymgo_amd_tactics.h')).read()
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
    return hdr, decls


def test_tactics_binding_table_matches_its_header(native_built):
    import ctypes
    import test_host_abi as tha
    from gymgo_amd import _lib
    hdr, decls = tactics_declarations()
    assert list(decls) == ['gg_tactics_planes', 'gg_batch_tactics', 'gg_batch_tactics_tracked', 'gg_batch_rollout_tracked_policy2',
                           'gg_playouts_advance_policy2', 'gg_move_playouts_advance_policy2']
    assert tha._abi_mismatches(decls, _lib.ABI_TACTICS) == []
    assert _lib.EXPORTS_TACTICS == tuple(decls) and not set(decls) & set(_lib.EXPORTS)
    dropped = dict(_lib.ABI_TACTICS, gg_batch_tactics=_lib.ABI_TACTICS['gg_batch_tactics'][:1] + _lib.ABI_TACTICS['gg_batch_tactics'][2:])
    assert any('7 parameters in the header, 6 in the table' in b for b in tha._abi_mismatches(decls, dropped))   # the comparison can fail
    # the _policy2 calls take the parameter lists of their namesakes
    for f in ('gg_batch_rollout_tracked_policy', 'gg_playouts_advance_policy', 'gg_move_playouts_advance_policy'):
        assert _lib.ABI_TACTICS[f + '2'] == _lib.ABI[f]
    for f, (argtypes, restype) in _lib._SIGNATURES_TACTICS.items():
        assert restype is ctypes.c_int32
        assert argtypes == [p.kind if isinstance(p.kind, type) else ctypes.c_void_p for p in _lib.ABI_TACTICS[f]]
    L = ctypes.CDLL(_lib.LIB_PATH)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in list(decls) + ['GG_POLICY_TACTICAL', 'gymgo_amd_tactics.h']:
        assert name in doc, name
    for name in decls:
        assert hasattr(L, name), name
    assert '#define GG_POLICY_TACTICAL 2' in hdr
    assert native_built.gg_tactics_planes() == 3 and native_built.gg_version() == _lib.ABI_VERSION == 5


def test_policy2_entry_points_check_arguments_in_the_order_of_their_namesakes(built):
    """Pointers that are never followed: every call below returns from its checks."""
    L = built.lib()

    def rollout(fn, policy=2, plies=1, B=4, N=9, ptr=1):
        q = ptr or None
        return fn(q, q, None, None, B, N, plies, 0, policy, None)

    def po(fn, policy=2, chunks=1, N=9, K=2, ptr=1):
        q = ptr or None
        return fn(q, 4, N, K, 0, 7, 64, 32, 0.0, chunks, policy, q, q, q, q, 8, q, q, q, None, None)

    def mvp(fn, policy=2, chunks=1, N=9, K=2, ptr=1):
        q = ptr or None
        return fn(q, 4, N, q, 3, K, 0, 7, 64, 32, 0.0, chunks, policy, q, q, q, q, 8, q, q, q, None)

    fams = ((rollout, L.gg_batch_rollout_tracked_policy2, L.gg_batch_rollout_tracked_policy),
            (po, L.gg_playouts_advance_policy2, L.gg_playouts_advance_policy),
            (mvp, L.gg_move_playouts_advance_policy2, L.gg_move_playouts_advance_policy))
    for call, new, old in fams:
        assert call(new, policy=3) == -3 and call(new, policy=-1) == -3 and call(new, policy=1 << 20) == -3
        assert call(old, policy=2) == -3                                  # the namesakes keep refusing the new policy
        assert call(new, N=1) == -1 and call(new, N=20) == -1
        assert call(new, ptr=0) == -2
        # every refusal of the namesake, with a policy both accept or both refuse, is the new call's refusal too
        for policy in (0, 1, -1, 7):
            for kw in ({'N': 1}, {'N': 20}, {'ptr': 0}, {'N': 20, 'ptr': 0}):
                assert call(new, policy=policy, **kw) == call(old, policy=policy, **kw) != 0, (call.__name__, policy, kw)
    new, old = fams[0][1:]
    assert rollout(new, plies=-1) == -3 and rollout(new, B=-1) == -1 and rollout(new, B=0) == 0
    assert rollout(new, plies=-1, N=20) == -3 and rollout(new, policy=7, N=20) == -3      # the policy and plies before the sizes
    assert rollout(new, plies=0, ptr=0) == -2
    for policy in (0, 1):
        for kw in ({'plies': -1}, {'B': -1}, {'B': 0}, {'plies': -1, 'N': 20}):
            assert rollout(new, policy=policy, **kw) == rollout(old, policy=policy, **kw)
    for call, new, old in fams[1:]:
        assert call(new, K=0) == -3 and call(new, chunks=-1) == -3
        assert call(new, policy=7, N=20) == -1 and call(new, policy=7, ptr=0) == -2       # the queue's checks before the policy
        assert call(new, chunks=0) == 0 and call(new, policy=7, chunks=0) == -3
        for policy in (0, 1, 7):
            for kw in ({'K': 0}, {'chunks': -1}, {'chunks': 0}):
                assert call(new, policy=policy, **kw) == call(old, policy=policy, **kw)
    # the planes: plane_launch's checks
    for fn in (L.gg_batch_tactics, L.gg_batch_tactics_tracked):
        assert fn(16, None, 16, 3, 4, 1, None) == -1 and fn(16, None, 16, 3, 4, 20, None) == -1
        assert fn(16, None, 16, 3, -1, 9, None) == -1 and fn(16, None, 16, 4, 4, 9, None) == -1 and fn(16, None, 16, -1, 4, 9, None) == -1
        assert fn(None, None, None, 3, 0, 9, None) == 0
        assert fn(None, None, 16, 3, 4, 9, None) == -2 and fn(16, None, None, 3, 4, 9, None) == -2
        assert fn(16, None, 18, 0, 4, 9, None) == -3 and fn(16, None, 17, 1, 4, 9, None) == -3


def test_python_api_policy_names_and_value_errors():
    from gymgo_amd import gogame
    assert gogame.POLICIES == {'uniform': 0, 'no_eye_fill': 1}
    assert gogame.PLAYOUT_POLICIES == {'uniform': 0, 'no_eye_fill': 1, 'tactical': 2}
    assert [gogame._policy_code(k) for k in ('uniform', 'no_eye_fill', 'tactical')] == [0, 1, 2]
    assert gogame.TACTICS_NAMES == ('capture', 'escape', 'no_eye_fill') and gogame.TACTICS_PLANES == 3
    st = np.zeros((2, 6, 5, 5), np.uint8)
    for bad in ('Tactical', 'tactics', 2, None, b'tactical'):
        with pytest.raises(ValueError):
            gogame._policy_code(bad)
        with pytest.raises(ValueError):
            gogame.batch_playouts(st, 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.playouts(st[0], 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.batch_move_playouts(st, 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.move_playouts(st[0], 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.flat_mc_actions(st, 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.batch_uct(st, 2, 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.uct(st[0], 2, 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.uct_actions(st, 2, 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.playout_evaluator(2, policy=bad, komi=0.5)
        with pytest.raises(ValueError):
            gogame.batch_rollout_tracked(None, None, 1, policy=bad)
    # the plane calls: every ValueError before a device is touched
    import torch
    with pytest.raises(ValueError):
        gogame.batch_tactics(np.zeros((2, 6, 5, 4), np.uint8))
    with pytest.raises(ValueError):
        gogame.batch_tactics(st, dtype=torch.int32)
    with pytest.raises(ValueError):
        gogame.batch_tactics(st, orient=[0])
    with pytest.raises(ValueError):
        gogame.batch_tactics_tracked(np.zeros((2, 26), np.int32))
    if not torch.cuda.is_available():     # ... and there is no CPU path
        from gymgo_amd import _lib
        with pytest.raises(_lib.GymGoNativeError):
            gogame.batch_tactics(st)
        with pytest.raises(_lib.GymGoNativeError):
            gogame.tactics(st[0])
