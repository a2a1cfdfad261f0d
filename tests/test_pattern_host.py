"""CPU: the `pattern` playout policy without a device - the thirteen patterns (mc_pattern_expect.pattern_tables) against the
counts of their header, their symmetries and hand-made positions point by point, the committed table of the kernels
(gymgo_amd/csrc/gg_pattern_tab.h) against the restatement, the properties of the ply-by-ply expectation
(mc_pattern_expect.pattern_rollout) that the GPU tests compare against, with the premises of every GPU case, the binding table
of the family (_lib.ABI_PATTERN) against its header, and the argument checks of the Python API and the C entry points."""
import os
import re

import numpy as np
import pytest

import mc_expect as mc
import mc_pattern_expect as mq
import mc_tactics_expect as mt
from oracle import c_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built(native_built):
    from gymgo_amd import _lib
    return _lib


def test_checksum_counts_of_the_thirteen_patterns():
    t = mq.pattern_tables()
    assert t.shape == (13, 4 ** 8)
    assert tuple(int(x) for x in t.sum(axis=1)) == mq.COUNTS == (504, 256, 768, 8, 4544, 3392, 2812, 10304, 240, 64, 608, 504, 64)
    assert int(t.any(axis=0).sum()) == mq.TOTAL == 15828
    hdr = open(os.path.join(ROOT, 'include', 'gymgo_amd_pattern.h')).read()
    for p in mq.PATTERNS:
        assert p in hdr, p
    assert '15 828' in hdr and '504, 256, 768, 8, 4 544, 3 392, 2 812, 10 304, 240, 64, 608, 504, 64' in hdr


def _table_index(code):
    """The index pattern_index (gymgo_amd/csrc/gg_common.h) forms for the neighbourhood `code` of mc_pattern_expect, with black
    as the mover: two bits per neighbour - "mover or off", "opponent or off" - laid out as tools/gen_pattern_table.py documents."""
    bits = ((0, 3), (1, 4), (2, 5), (6, 8), (7, 9), (10, 13), (11, 14), (12, 15))
    i = 0
    for j, (bm, bo) in enumerate(bits):
        s = (code >> (2 * j)) & 3
        if s in (mq.BLACK, mq.OFF):
            i |= 1 << bm
        if s in (mq.WHITE, mq.OFF):
            i |= 1 << bo
    return i


def test_committed_table_of_the_kernels_equals_the_restatement():
    src = open(os.path.join(ROOT, 'gymgo_amd', 'csrc', 'gg_pattern_tab.h')).read()
    words = [int(w, 16) for w in re.findall(r'0x([0-9A-F]{8})u', src)]
    assert len(words) == 2048
    bits = np.array([(words[i >> 5] >> (i & 31)) & 1 for i in range(1 << 16)], bool)
    assert int(bits.sum()) == mq.TOTAL
    want = mq.match_table()
    idx = np.array([_table_index(c) for c in range(4 ** 8)])
    assert len(set(idx.tolist())) == 4 ** 8                         # the index is a bijection of the neighbourhoods
    assert np.array_equal(bits[idx], want)


def test_pattern_points_are_invariant_under_the_eight_views_and_a_colour_swap():
    for N in (2, 3, 5, 9):
        roots = mt.pool(N)
        P = mq.pattern_points(roots)
        sw = roots.copy()
        sw[:, 0], sw[:, 1] = roots[:, 1], roots[:, 0]
        assert np.array_equal(mq.pattern_points(sw), P), N
        tm = roots.copy()
        tm[:, 2] = 1 - roots[:, 2]                                  # ... nor on who is to move
        assert np.array_equal(mq.pattern_points(tm), P), N
        for k in range(4):
            for flip in (False, True):
                v = np.rot90(roots, k, axes=(2, 3))
                w = np.rot90(P, k, axes=(1, 2))
                if flip:
                    v, w = v[:, :, :, ::-1], w[:, :, ::-1]
                assert np.array_equal(mq.pattern_points(np.ascontiguousarray(v)), w), (N, k, flip)
        assert P.any() or N == 2


def test_sets_on_hand_made_positions_point_by_point():
    pos = mq.crafted_positions()
    assert [p[0] for p in pos][::2] == ['hane_row', 'pair', 'cut', 'edge', 'two_by_two']
    for name, b, prev, P, L in pos:
        N = b.shape[-1]
        last = None if prev is None else np.array([prev[0] * N + prev[1]], np.int32)
        gp, gl = mq.pattern_sets(b[None], last)
        for y in range(N):
            for x in range(N):
                assert bool(gp[0, y, x]) == bool(P[y, x]), (name, 'P', y, x)
                assert bool(gl[0, y, x]) == bool(L[y, x]), (name, 'L', y, x)
        # no previous point: -1, the pass, anything else
        for v in (-1, N * N, -7, 1 << 30):
            assert not mq.pattern_sets(b[None], np.array([v], np.int32))[1].any(), (name, v)
        e = b.copy()
        e[5] = 1
        assert not any(s.any() for s in mq.pattern_sets(e[None], last)), name     # a game that has ended


def _check_trace(trace, N):
    for live, before, n, act, which, gate, onlyL, prev, Lp in trace:
        C, E, F = mt.tiers(before)
        P = mq.pattern_points(before)
        pt = act < N * N
        assert np.array_equal(~pt, n == 0) and not (~pt & (which != mq.SET_F)).any()
        assert not (Lp & ~F).any() and not (Lp & ~P).any()
        for i in np.flatnonzero(which == mq.SET_L):
            y, x = divmod(int(act[i]), N)
            py, px = divmod(int(prev[i]), N)
            assert gate[i] and not C[i].any() and not E[i].any() and Lp[i, y, x]
            assert 0 <= prev[i] < N * N and max(abs(y - py), abs(x - px)) == 1
        assert not (Lp.reshape(len(live), -1).any(axis=1) & ((prev < 0) | (prev >= N * N))).any()


def test_pattern_rollout_properties_9x9_and_the_recorded_counts():
    N, B = 9, 64
    st = np.zeros((B, 6, N, N), np.uint8)
    rng0 = c_oracle.rng_seed(1, B)
    trace = []
    fin, rng1, last, steps = mq.pattern_rollout(st, rng0, 8 * N * N, auto_reset=False, trace=trace)
    _check_trace(trace, N)
    assert np.array_equal(mc.plies_from_rng(rng0, rng1), steps)
    assert (fin[:, 5, 0, 0] == 1).all() and steps.max() < 8 * N * N          # every one of the 64 games ended
    assert (last == N * N).all()
    got = mq.trace_counts(trace)
    # (the issue's prototype, 512 games: 11 302 plies from C, 1 196 from E, 11 848 from L, 32 251 from F - L about one ply in five)
    assert got['L'] * 10 >= got['plies'] and got['C'] >= 500 and got['E'] >= 50, got
    assert got['open_L_only'] >= got['L'] > 0 and got['after_pass'] > 0
    assert got['C'] + got['E'] + got['L'] + got['F'] == got['plies'] == int(steps.sum())
    # ... and the policy is not the tactical one
    fin2, _, _, _ = mt.tactical_rollout(st, rng0, 8 * N * N, auto_reset=False)
    assert not np.array_equal(fin, fin2)


@pytest.mark.parametrize('N', [2, 3, 4, 5, 6, 7, 13])
def test_pattern_games_end_at_every_size(N):
    B = 16
    rng0 = c_oracle.rng_seed(1, B)
    trace = []
    fin, rng1, last, steps = mq.pattern_rollout(np.zeros((B, 6, N, N), np.uint8), rng0, 8 * N * N, auto_reset=False, trace=trace)
    if N <= 5:
        _check_trace(trace, N)
    assert (fin[:, 5, 0, 0] == 1).all() and steps.max() < 8 * N * N, (N, int(steps.max()))
    assert np.array_equal(mc.plies_from_rng(rng0, rng1), steps)
    if N >= 3:
        assert mq.trace_counts(trace)['L'] > 0


def test_pattern_games_end_on_19x19():
    N, B = 19, 6
    rng0 = c_oracle.rng_seed(1, B)
    fin, rng1, last, steps = mq.pattern_rollout(np.zeros((B, 6, N, N), np.uint8), rng0, 8 * N * N, auto_reset=False)
    assert (fin[:, 5, 0, 0] == 1).all() and steps.max() < 8 * N * N, int(steps.max())
    assert np.array_equal(mc.plies_from_rng(rng0, rng1), steps)


def test_carried_last_makes_launches_of_any_lengths_one_launch():
    for N, auto in ((5, False), (5, True), (9, True)):
        st, last0 = mq.rollout_batch(N, 40)
        rng0 = c_oracle.rng_seed(5, len(st))
        whole = mq.pattern_rollout(st, rng0, 50, auto_reset=auto, last=last0)
        cur, rng, last = st, rng0, last0
        for n in (1, 2, 7, 8, 32):
            cur, rng, out, _ = mq.pattern_rollout(cur, rng, n, auto_reset=auto, last=last)
            last = out          # (as the kernels write it: -1 for a board that did not play - it is frozen for good, or absent)
        assert np.array_equal(cur, whole[0]) and np.array_equal(rng, whole[1]), (N, auto)


def test_premises_of_the_gpu_cases():
    """What tests/test_gpu_pattern.py relies on: every lockstep case draws from L, sees an open gate with C and E empty and L not
    empty, and a previous pass; at 19x19 L crosses the seam between rows 9 and 10 in both directions."""
    for N in (2, 3, 5, 9):
        st, last = mq.rollout_batch(N, 64)
        trace = []
        mq.pattern_rollout(st, c_oracle.rng_seed(11, 64), 50, auto_reset=True, last=last, trace=trace)
        got = mq.trace_counts(trace)
        if N > 2:
            assert got['L'] > 0 and got['open_L_only'] > 0, (N, got)
        assert got['after_pass'] > 0, (N, got)
        P, L = mq.pattern_sets(st, last)
        assert L.any() or N == 2, N
        assert not L[(last < 0) | (last >= N * N)].any()
    roots, last = mq.seam_roots()
    P, L = mq.pattern_sets(roots, last)
    assert L.reshape(len(roots), -1).any(axis=1).all()                            # every seam root has a local response
    prow = last // 19
    up = (prow == 10) & L[:, 9].any(axis=1)                                       # the move in row 10, a response in row 9
    down = (prow == 9) & L[:, 10].any(axis=1)                                     # ... and the other way round
    assert up.any() and down.any()
    pcol = last % 19
    for edge in (prow == 0, prow == 18, pcol == 0, pcol == 18, (prow % 18 == 0) & (pcol % 18 == 0)):
        assert edge.any()                                                         # (each with a response: the line above)
    st19, l19 = mq.rollout_batch(19, 64)
    trace = []
    mq.pattern_rollout(st19, c_oracle.rng_seed(11, 64), 8, auto_reset=True, last=l19, trace=trace)
    got = mq.trace_counts(trace)
    assert got['L'] > 0 and got['open_L_only'] > 0, got
    seam_hit = False
    for live, before, n, act, which, gate, onlyL, prev, Lp in trace:
        sel = (which == mq.SET_L) & (prev >= 0)
        seam_hit |= bool((sel & (prev // 19 == 9) & (act // 19 == 10)).any() or (sel & (prev // 19 == 10) & (act // 19 == 9)).any())
    assert seam_hit                                                               # a drawn response crosses the seam


def test_expected_pattern_results_are_consistent():
    N, R, K = 5, 6, 4
    roots = mc.make_roots(N, R, 9, max_ply=24, step=4)
    full = mq.expected_playouts_pattern(roots, K, 8 * N * N, with_ownership=True)
    assert np.array_equal(full['black_wins'] + full['white_wins'] + full['draws'], np.full(R, K))
    a = mq.expected_playouts_pattern(roots[:2], K, 8 * N * N, first_root=0)
    b = mq.expected_playouts_pattern(roots[2:], K, 8 * N * N, first_root=2)
    for k in ('black_wins', 'margin_sum', 'plies_sum'):
        assert np.array_equal(np.concatenate([a[k], b[k]]), full[k])
    t = mt.expected_playouts_tactical(roots, K, 8 * N * N)
    assert not np.array_equal(t['plies_sum'], full['plies_sum'])                  # not the tactical playouts
    mv = mq.expected_move_playouts_pattern(roots[:2], 2, 8 * N * N)
    assert np.array_equal(mv['legal'], mc.legal_mask(roots[:2]))
    u = mq.expected_uct_pattern(roots[:2], 3, 2)
    assert (u['root_visits'] == 6).all()


# ---------------------------------------------------------------- the family's header against its binding table
def pattern_declarations():
    """{function: [(C type without const, is pointer, parameter name)]} of every `int32_t gg_*(...);` of
    include/gymgo_amd_pattern.h, in header order (test_tactics_host.tactics_declarations, of this header)."""
    hdr = open(os.path.join(ROOT, 'include', 'gymgo_amd_pattern.h')).read()
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


def test_pattern_binding_table_matches_its_header(native_built):
    import ctypes
    import test_host_abi as tha
    from gymgo_amd import _lib
    hdr, decls = pattern_declarations()
    assert list(decls) == ['gg_pattern_planes', 'gg_batch_patterns', 'gg_batch_patterns_tracked', 'gg_batch_rollout_tracked_policy3',
                           'gg_playouts_advance_policy3', 'gg_move_playouts_advance_policy3']
    assert tha._abi_mismatches(decls, _lib.ABI_PATTERN) == []
    assert _lib.EXPORTS_PATTERN == tuple(decls) and not set(decls) & (set(_lib.EXPORTS) | set(_lib.EXPORTS_TACTICS))
    dropped = dict(_lib.ABI_PATTERN, gg_batch_patterns=_lib.ABI_PATTERN['gg_batch_patterns'][:1] + _lib.ABI_PATTERN['gg_batch_patterns'][2:])
    assert any('8 parameters in the header, 7 in the table' in b for b in tha._abi_mismatches(decls, dropped))   # the comparison can fail
    # the rollout takes the parameter list of _policy2, the queue calls theirs plus `last` in front of the stream
    assert _lib.ABI_PATTERN['gg_batch_rollout_tracked_policy3'] == _lib.ABI_TACTICS['gg_batch_rollout_tracked_policy2']
    for f in ('gg_playouts_advance_policy', 'gg_move_playouts_advance_policy'):
        new, old = _lib.ABI_PATTERN[f + '3'], _lib.ABI_TACTICS[f + '2']
        assert new[:-2] == old[:-1] and new[-1] == old[-1] and new[-2].name == 'last'
    for f, (argtypes, restype) in _lib._SIGNATURES_PATTERN.items():
        assert restype is ctypes.c_int32
        assert argtypes == [p.kind if isinstance(p.kind, type) else ctypes.c_void_p for p in _lib.ABI_PATTERN[f]]
    L = ctypes.CDLL(_lib.LIB_PATH)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in list(decls) + ['GG_POLICY_PATTERN', 'gymgo_amd_pattern.h']:
        assert name in doc, name
    for name in decls:
        assert hasattr(L, name), name
    assert '#define GG_POLICY_PATTERN 3' in hdr
    assert native_built.gg_pattern_planes() == 2 and native_built.gg_version() == _lib.ABI_VERSION == 5


def test_policy3_entry_points_check_arguments_in_the_order_of_their_namesakes(built):
    """Pointers that are never followed: every call below returns from its checks."""
    L = built.lib()

    def rollout(fn, policy=3, plies=1, B=4, N=9, ptr=1, last=1):
        q = ptr or None
        return fn(q, q, last or None, None, B, N, plies, 0, policy, None)

    def po(fn, policy=3, chunks=1, N=9, K=2, ptr=1, last=1, three=True):
        q = ptr or None
        tail = ((last or None), None) if three else (None,)
        return fn(q, 4, N, K, 0, 7, 64, 32, 0.0, chunks, policy, q, q, q, q, 8, q, q, q, None, *tail)

    def mvp(fn, policy=3, chunks=1, N=9, K=2, ptr=1, last=1, three=True):
        q = ptr or None
        tail = ((last or None), None) if three else (None,)
        return fn(q, 4, N, q, 3, K, 0, 7, 64, 32, 0.0, chunks, policy, q, q, q, q, 8, q, q, q, *tail)

    new, old = L.gg_batch_rollout_tracked_policy3, L.gg_batch_rollout_tracked_policy2
    assert rollout(new, policy=4) == -3 and rollout(new, policy=-1) == -3 and rollout(new, policy=1 << 20) == -3
    assert rollout(old, policy=3) == -3                                   # the namesake keeps refusing the new policy
    assert rollout(new, N=1) == -1 and rollout(new, N=20) == -1 and rollout(new, ptr=0) == -2
    assert rollout(new, plies=-1) == -3 and rollout(new, B=-1) == -1 and rollout(new, B=0) == 0
    assert rollout(new, plies=-1, N=20) == -3 and rollout(new, policy=7, N=20) == -3       # the policy and plies before the sizes
    assert rollout(new, plies=0, ptr=0) == -2 and rollout(new, plies=0, last=0) == 0
    assert rollout(new, last=0) == -2                                     # policy 3 needs last_actions ...
    assert rollout(new, last=0, N=20) == -1 and rollout(new, last=0, plies=-1) == -3       # ... after every check of the namesake
    for policy in (0, 1, 2, -1, 7):
        for kw in ({'N': 1}, {'N': 20}, {'ptr': 0}, {'N': 20, 'ptr': 0}, {'plies': -1}, {'B': -1}, {'B': 0}, {'plies': -1, 'N': 20}):
            assert rollout(new, policy=policy, **kw) == rollout(old, policy=policy, **kw), (policy, kw)
    for call, new, old in ((po, L.gg_playouts_advance_policy3, L.gg_playouts_advance_policy2),
                           (mvp, L.gg_move_playouts_advance_policy3, L.gg_move_playouts_advance_policy2)):
        assert call(new, policy=4) == -3 and call(new, policy=-1) == -3 and call(old, policy=3, three=False) == -3
        assert call(new, N=1) == -1 and call(new, N=20) == -1 and call(new, ptr=0) == -2
        assert call(new, K=0) == -3 and call(new, chunks=-1) == -3
        assert call(new, policy=7, N=20) == -1 and call(new, policy=7, ptr=0) == -2         # the queue's checks before the policy
        assert call(new, chunks=0) == 0 and call(new, policy=7, chunks=0) == -3
        assert call(new, last=0) == -2 and call(new, last=0, chunks=0) == -2                # policy 3 needs last, after the policy check
        assert call(new, last=0, chunks=-1) == -3 and call(new, last=0, N=20) == -1 and call(new, last=0, K=0) == -3
        for policy in (0, 1, 2, 7):
            for kw in ({'K': 0}, {'chunks': -1}, {'chunks': 0}, {'N': 20}, {'ptr': 0}):
                assert call(new, policy=policy, last=0, **kw) == call(old, policy=policy, three=False, **kw), (policy, kw)
    # the planes: plane_launch's checks
    for fn in (L.gg_batch_patterns, L.gg_batch_patterns_tracked):
        assert fn(16, None, None, 16, 3, 4, 1, None) == -1 and fn(16, None, None, 16, 3, 4, 20, None) == -1
        assert fn(16, None, None, 16, 3, -1, 9, None) == -1 and fn(16, None, None, 16, 4, 4, 9, None) == -1
        assert fn(16, None, None, 16, -1, 4, 9, None) == -1
        assert fn(None, None, None, None, 3, 0, 9, None) == 0
        assert fn(None, None, None, 16, 3, 4, 9, None) == -2 and fn(16, None, None, None, 3, 4, 9, None) == -2
        assert fn(16, None, None, 18, 0, 4, 9, None) == -3 and fn(16, None, None, 17, 1, 4, 9, None) == -3


def test_python_api_policy_names_and_value_errors():
    import torch
    from gymgo_amd import gogame
    assert gogame.POLICIES == {'uniform': 0, 'no_eye_fill': 1}
    assert gogame.PLAYOUT_POLICIES == {'uniform': 0, 'no_eye_fill': 1, 'tactical': 2}       # unchanged
    assert gogame.LOCAL_PLAYOUT_POLICIES == {'pattern': 3}
    assert [gogame._policy_code(k) for k in ('uniform', 'no_eye_fill', 'tactical', 'pattern')] == [0, 1, 2, 3]
    assert gogame.PATTERN_NAMES == ('pattern', 'local') and gogame.PATTERN_PLANES == 2
    st = np.zeros((2, 6, 5, 5), np.uint8)
    for bad in ('Pattern', 'patterns', 3, None, b'pattern'):
        with pytest.raises(ValueError):
            gogame._policy_code(bad)
        with pytest.raises(ValueError):
            gogame.batch_playouts(st, 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.batch_rollout_tracked(None, None, 1, policy=bad)
    # the move log has no pattern variants: ValueError before a device is touched
    with pytest.raises(ValueError):
        gogame.batch_playouts(st, 2, policy='pattern', amaf=True)
    with pytest.raises(ValueError):
        gogame.playouts(st[0], 2, policy='pattern', amaf=True)
    with pytest.raises(ValueError):
        gogame.batch_uct(st, 2, 2, policy='pattern', rave_equiv=8.0)
    with pytest.raises(ValueError):
        gogame.uct_actions(st, 2, 2, policy='pattern', rave_equiv=8.0)
    with pytest.raises(ValueError):
        gogame.batch_rollout_tracked_log(None, None, 1, None, policy='pattern')
    # the plane calls: every ValueError before a device is touched
    with pytest.raises(ValueError):
        gogame.batch_patterns(np.zeros((2, 6, 5, 4), np.uint8))
    with pytest.raises(ValueError):
        gogame.batch_patterns(st, dtype=torch.int32)
    with pytest.raises(ValueError):
        gogame.batch_patterns(st, orient=[0])
    with pytest.raises(ValueError):
        gogame.batch_patterns(st, last=[0])
    with pytest.raises(ValueError):
        gogame.batch_patterns(st, last=[0.5, 1.0])
    with pytest.raises(ValueError):
        gogame.batch_patterns_tracked(np.zeros((2, 26), np.int32))
    if not torch.cuda.is_available():     # ... and there is no CPU path
        from gymgo_amd import _lib
        with pytest.raises(_lib.GymGoNativeError):
            gogame.batch_patterns(st)
        with pytest.raises(_lib.GymGoNativeError):
            gogame.patterns(st[0], 7)
        with pytest.raises(_lib.GymGoNativeError):
            gogame.batch_playouts(st, 2, policy='pattern')
