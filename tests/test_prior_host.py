"""CPU: the move priors of the RAVE search without a device - the binding table of the family (_lib.ABI_PRIOR) against its header,
the argument checks of the C entry points and of the Python API (every ValueError before a device is touched), the rule of
tests/mc_prior_expect.py on hand-made positions, and the premises of every case tests/test_gpu_prior.py runs."""
import ctypes
import math
import os

import numpy as np
import pytest

import mc_pattern_expect as mq
import mc_prior_expect as me
import mc_tactics_expect as mt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['gg_batch_move_priors', 'gg_batch_move_priors_tracked', 'gg_uct_prior_begin', 'gg_uct_prior_expand']


@pytest.fixture(scope='module')
def built(native_built):
    from gymgo_amd import _lib
    return _lib


# ---------------------------------------------------------------- the family's header against its binding table
def test_prior_binding_table_matches_its_header(native_built):
    import test_host_abi as tha
    from gymgo_amd import _lib
    decls = tha.header_declarations('gymgo_amd_prior.h')
    assert list(decls) == NAMES
    assert tha._abi_mismatches(decls, _lib.ABI_PRIOR) == []
    assert _lib.EXPORTS_PRIOR == tuple(decls)
    others = (_lib.EXPORTS, _lib.EXPORTS_AREA, _lib.EXPORTS_PAST, _lib.EXPORTS_GUMBEL, _lib.EXPORTS_TACTICS, _lib.EXPORTS_AMAF,
              _lib.EXPORTS_PATTERN)
    assert not set(decls) & {f for t in others for f in t}                      # no name in common with the other tables
    dropped = dict(_lib.ABI_PRIOR, gg_uct_prior_begin=_lib.ABI_PRIOR['gg_uct_prior_begin'][1:])
    assert any('8 parameters in the header, 7 in the table' in b for b in tha._abi_mismatches(decls, dropped))   # the comparison can fail
    for f, (argtypes, restype) in _lib._SIGNATURES_PRIOR.items():               # the ctypes signatures come from the table
        assert restype is ctypes.c_int32
        assert argtypes == [p.kind if isinstance(p.kind, type) else ctypes.c_void_p for p in _lib.ABI_PRIOR[f]]
        assert _lib._POINTERS[f][0] == len(_lib.ABI_PRIOR[f])
    # const: everything but the two outputs
    for f, ps in tha.header_declarations('gymgo_amd_prior.h', const=True).items():
        for ctype, pointer, name, const in ps:
            if pointer and name != 'hip_stream':
                assert const == (name not in ('out', 'node_amaf')), (f, name)
    L = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, 'include', 'gymgo_amd_prior.h')).read()
    assert '0 <= wins <= visits' in hdr and '< 2^31' in hdr                     # the contract of the weights and the bound
    for doc in ('INTEGRATION.md', 'README.md'):
        text = open(os.path.join(ROOT, doc)).read()
        for name in NAMES + ['gymgo_amd_prior.h']:
            assert name in text, (doc, name)
    for name in decls:
        assert hasattr(L, name), name
    assert native_built.gg_version() == _lib.ABI_VERSION == 5                   # additive: the ABI version stays


def test_entry_points_check_arguments_in_order(built):
    """Pointers that are never followed: every call below returns from its checks."""
    L = built.lib()
    for fn in (L.gg_batch_move_priors, L.gg_batch_move_priors_tracked):
        assert fn(16, None, 16, 16, 4, 1, None) == -1 and fn(16, None, 16, 16, 4, 20, None) == -1 and fn(16, None, 16, 16, -1, 9, None) == -1
        assert fn(None, None, None, None, 0, 9, None) == 0                      # B = 0 is no work
        assert fn(None, None, None, None, 0, 20, None) == -1
        assert fn(None, None, 16, 16, 4, 9, None) == -2 and fn(16, None, None, 16, 4, 9, None) == -2 and fn(16, None, 16, None, 4, 9, None) == -2
        assert fn(16, None, 16, 18, 4, 9, None) == -3 and fn(16, 16, 16, 17, 4, 9, None) == -3

    def begin(R=4, N=9, I=3, roots=16, last=None, weights=16, amaf=16):
        return L.gg_uct_prior_begin(roots, last, R, N, I, weights, amaf, None)

    def expand(R=4, N=9, I=3, weights=16, leaf=16, move=16, leaf_id=16, amaf=16):
        return L.gg_uct_prior_expand(R, N, I, weights, leaf, move, leaf_id, amaf, None)

    for call in (begin, expand):
        assert call(N=1) == -1 and call(N=20) == -1 and call(R=-1) == -1
        assert call(I=0) == -3 and call(I=2 ** 31 - 1) == -3 and call(N=20, I=0) == -1      # the sizes before the arguments
        assert call(weights=None) == -2 and call(amaf=None) == -2 and call(I=0, amaf=None) == -3
        assert call(R=0) == 0 and call(R=0, amaf=None) == -2                                # the pointers before "no work", as the RAVE calls
        assert call(amaf=18) == -3
    assert begin(roots=None) == -2
    for name in ('leaf', 'move', 'leaf_id'):
        assert expand(**{name: None}) == -2


# ---------------------------------------------------------------- the Python API
def test_python_api_names_and_the_documented_default():
    from gymgo_amd import gogame
    assert gogame.UctPrior._fields == me.TERMS == ('even', 'capture', 'escape', 'pattern', 'local', 'eye_fill')
    assert tuple(gogame.UCT_PRIOR) == tuple(me.DEFAULT) == ((8, 4), (8, 8), (8, 8), (4, 4), (8, 8), (16, 0))
    assert gogame._prior_arg(True) == gogame.UCT_PRIOR
    assert gogame._prior_arg([[1, 0], (2, 2), (3, 1), (0, 0), (np.int32(5), np.int64(5)), (7, 3)]) == ((1, 0), (2, 2), (3, 1), (0, 0), (5, 5), (7, 3))
    for doc in (gogame.batch_uct.__doc__, gogame.UctPrior.__doc__ + open(os.path.join(ROOT, 'DESIGN.md')).read()):
        assert 'untuned' in doc.lower()
    assert 'pass' in gogame.batch_uct.__doc__ and 'fpu' in gogame.batch_uct.__doc__
    for fn in (gogame.batch_move_priors, gogame.batch_move_priors_tracked, gogame.move_priors):
        assert callable(fn)


BAD_PRIORS = (False, 7, 'default', (), [(8, 4)] * 5, [(8, 4)] * 7, [(8, 4, 1)] * 6, [(4, 8)] * 6, [(8, -1)] * 6, [(-2, -2)] * 6,
              [(8.0, 4.0)] * 6, [(True, False)] * 6, [(2 ** 31, 0)] * 6, [8] * 6)


def test_every_value_error_comes_before_a_device_is_touched():
    """On the parent commit `prior=` is an unexpected keyword: TypeError, not ValueError."""
    from gymgo_amd import gogame
    st = np.zeros((2, 6, 5, 5), np.uint8)
    searches = ((gogame.batch_uct, st, 2), (gogame.uct_actions, st, 2), (gogame.uct, st[0], 1))
    for fn, s, R in searches:
        # prior or last_actions without rave_equiv
        with pytest.raises(ValueError):
            fn(s, 4, 2, prior=True)
        with pytest.raises(ValueError):
            fn(s, 4, 2, last_actions=[0] * R)
        with pytest.raises(ValueError):
            fn(s, 4, 2, rave_equiv=8.0, last_actions=[0] * R)               # ... nor last_actions without a prior
        with pytest.raises(ValueError):
            fn(s, 4, 2, prior=gogame.UCT_PRIOR, fpu=0.5)
        # malformed pairs
        for bad in BAD_PRIORS:
            with pytest.raises(ValueError):
                fn(s, 4, 2, rave_equiv=8.0, prior=bad)
        # 2 * (iterations * playouts + the visits) >= 2^31
        big = gogame.UctPrior((2 ** 30 - 8 - 6, 0), (1, 1), (1, 0), (1, 0), (1, 0), (2, 0))
        with pytest.raises(ValueError):
            fn(s, 4, 2, rave_equiv=8.0, prior=big)                              # 2 * (8 + 2^30 - 8) = 2^31
        with pytest.raises(ValueError):
            fn(s, 1 << 15, 1 << 15, rave_equiv=8.0, prior=True)                 # 2 * (2^30 + 52)
        # last_actions of the wrong length, or with an entry outside [-1, N^2]
        for bad in ([0] * (R + 1), [], [-2] * R, [26] * R, [0.0] * R, [True] * R):
            with pytest.raises(ValueError):
                fn(s, 4, 2, rave_equiv=8.0, prior=True, last_actions=bad)
    with pytest.raises(ValueError):
        gogame.batch_uct(np.zeros((2, 6, 5, 4), np.uint8), 4, 2, rave_equiv=8.0, prior=True)
    # the rule on its own
    for bad in BAD_PRIORS:
        for call in (lambda: gogame.batch_move_priors(st, bad), lambda: gogame.move_priors(st[0], bad),
                     lambda: gogame.batch_move_priors_tracked(None, bad)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        gogame.batch_move_priors(np.zeros((2, 6, 5, 4), np.uint8))
    with pytest.raises(ValueError):
        gogame.batch_move_priors(st, last=[0])
    with pytest.raises(ValueError):
        gogame.batch_move_priors(st, last=[0.5, 1.0])
    with pytest.raises(ValueError):
        gogame.batch_move_priors_tracked(np.zeros((2, 26), np.int32))
    import torch
    if not torch.cuda.is_available():     # ... and there is no CPU path: what passes the checks ends at the device
        from gymgo_amd import _lib
        with pytest.raises(_lib.GymGoNativeError):
            gogame.batch_move_priors(st)
        with pytest.raises(_lib.GymGoNativeError):
            gogame.batch_uct(st, 4, 2, rave_equiv=8.0, prior=True, last_actions=[-1, 25])
        with pytest.raises(_lib.GymGoNativeError):
            gogame.uct(st[0], 4, 2, rave_equiv=8.0, prior=gogame.UCT_PRIOR, last_actions=7)


def test_the_bound_counts_the_visits_of_the_prior():
    from gymgo_amd import gogame
    total = sum(v for v, _ in gogame.UCT_PRIOR)
    assert total == 52
    I, K = 1 << 15, 1 << 14                                                     # 2 I K = 2^30
    assert gogame._prior_kw({'prior': True, 'rave_equiv': 1.0}, 2, 5, I, K)[0] == gogame.UCT_PRIOR
    K2 = 1 << 15                                                                # 2 I K = 2^31: refused without the prior already
    with pytest.raises(ValueError):
        gogame._prior_kw({'prior': True, 'rave_equiv': 1.0}, 2, 5, I, K2)
    edge = gogame.UctPrior((2 ** 29 - 5, 0), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0))      # visits 2^29: 2 (2^29 + 2^29) = 2^31
    with pytest.raises(ValueError):
        gogame._prior_kw({'prior': edge, 'rave_equiv': 1.0}, 2, 5, I, K)
    ok = edge._replace(even=(2 ** 29 - 6, 0))
    assert gogame._prior_kw({'prior': ok, 'rave_equiv': 1.0}, 2, 5, I, K)[0] == ok
    pr, la = gogame._prior_kw({'prior': True, 'rave_equiv': 1.0, 'last_actions': np.array([-1, 25])}, 2, 5, 4, 2)
    assert la.dtype == np.int32 and la.tolist() == [-1, 25]
    assert gogame._prior_kw({'prior': None}, 2, 5, 4, 2) == (None, None)


# ---------------------------------------------------------------- the rule
def test_pairs_on_hand_made_positions_point_by_point():
    w = me.LOPSIDED
    for name, b, C, E in mt.crafted_positions():
        N = b.shape[-1]
        got = me.prior_pairs(b[None], None, w)[0].reshape(N, N, 2)
        F = mt.tiers(b[None])[2][0]
        P = mq.pattern_points(b[None])[0]
        for y in range(N):
            for x in range(N):
                if b[3, y, x]:
                    assert tuple(got[y, x]) == (0, 0), (name, y, x)
                    continue
                terms = [w.even] + [w.capture] * bool(C[y, x]) + [w.escape] * bool(E[y, x]) + [w.pattern] * bool(P[y, x]) \
                    + [w.eye_fill] * (not F[y, x])
                assert tuple(got[y, x]) == (sum(v for v, _ in terms), 2 * sum(s for _, s in terms)), (name, y, x)
        e = b.copy()
        e[5] = 1
        assert not me.prior_pairs(e[None], [0], w).any(), name                  # a game that has ended
    for name, b, prev, P, L in mq.crafted_positions():
        N = b.shape[-1]
        last = None if prev is None else [prev[0] * N + prev[1]]
        with_l = me.prior_pairs(b[None], last, w)[0].reshape(N, N, 2)
        without = me.prior_pairs(b[None], [-1], w)[0].reshape(N, N, 2)
        d = with_l - without
        assert np.array_equal(d[..., 0], L * w.local[0]) and np.array_equal(d[..., 1], L * 2 * w.local[1]), name
        for v in (N * N, -7, 1 << 30):
            assert np.array_equal(me.prior_pairs(b[None], [v], w)[0].reshape(N, N, 2), without), (name, v)


# ---------------------------------------------------------------- the premises of tests/test_gpu_prior.py
# the terms that occur on the boards of the small sizes (every one from 5x5 on): no group in atari has a last liberty with two
# empty neighbours on the 2x2 and 4x4 boards chosen
SMALL_TERMS = {2: ('even', 'capture', 'pattern', 'local', 'eye_fill'), 3: me.TERMS, 4: ('even', 'capture', 'pattern', 'local', 'eye_fill')}


def test_premises_of_the_pair_boards():
    for N in me.SIZES:
        st, last = me.pair_boards(N)
        assert 30 <= len(st) <= 70, (N, len(st))
        sets = me.prior_sets(st, last)
        occur = tuple(t for t, s in zip(me.TERMS, sets) if s.any())
        assert occur == (SMALL_TERMS[N] if N < 5 else me.TERMS), (N, occur)
        assert (st[:, 5, 0, 0] != 0).any()                                      # an ended board
        empty = (st[:, 0] == 0) & (st[:, 1] == 0)
        assert N < 4 or (empty & (st[:, 3] != 0) & (st[:, 5] == 0)).any()       # an empty point that is not legal: a ko (or a suicide)
        if N >= 3:
            assert (np.stack(sets[1:]).sum(axis=0) >= 3).any(), N               # a point in three sets at once
        assert ((last >= 0) & (last < N * N)).any() and (last == N * N).any() and (last < 0).any()
        for _, la in me.last_variants(N, len(st), last)[:3]:
            assert not me.prior_sets(st, la)[4].any()                           # no previous point: no L
    ko = mt.crafted_positions()[-1]
    assert ko[0] == 'ko_point_not_in_C' and any(np.array_equal(ko[1], b) for b in me.pair_boards(5)[0])
    st, last = me.mixed_boards(533)
    assert len(st) == 533 and me.prior_pairs(st[:80], last[:80], me.DEFAULT).any()


def test_premises_of_the_tree_cases():
    """Small sizes here (the 19x19 cases take seconds each on the CPU and run with the device test): a root's tree under the
    prior differs from the same search without one in its first expanded action and in its child tables, a root with
    last_actions differs from the same root with none, and the crafted root tries its capture first."""
    for N in (2, 5, 9):
        roots, last = me.tree_roots(N)
        assert len(roots) == 5 and (roots[3, 5] != 0).all()
        assert me.prior_sets(roots[4:], None)[1].any()                          # the crafted root has a capture
    N = 5
    plain = me.rave_case(N, 0.0)
    for c, prior, with_last in ((0.0, 'default', False), (0.0, 'default', True), (0.0, 'lopsided', False)):
        got = me.tree_case(N, c, prior, with_last)
        first_plain = [int(t.action[1]) if len(t.boards) > 1 else None for t in plain['trees']]
        assert got['first'][3] is None and first_plain[3] is None               # the finished game expands nothing
        differ = [r for r in range(5) if got['first'][r] != first_plain[r] and not np.array_equal(got['tree']['child'][r], plain['trees'][r].child)]
        assert differ, (prior, with_last)
        # the crafted root starts with its capture (2, 3) or its escape (2, 0), not with point 0: equal pairs under the default, ties
        # to the lowest point; the capture is also the local answer to the previous move, and the lopsided prior puts it first
        assert got['first'][4] == (2 * N if (prior, with_last) == ('default', False) else 2 * N + 3) and first_plain[4] == 0
        seeded = me.prior_pairs(me.tree_roots(N)[0], me.tree_roots(N)[1] if with_last else None, me.PRIORS[prior])
        assert (got['rave_visits'] >= seeded[:, :, 0]).all() and seeded[[0, 1, 2, 4]].any(axis=(1, 2)).all()    # the result includes the root's prior
    a, b = me.tree_case(N, 0.0, 'default', True), me.tree_case(N, 0.0, 'default', False)
    roots, last = me.tree_roots(N)
    assert me.prior_sets(roots, last)[4].any()                                  # some root has a local answer to its previous move ...
    assert any(not np.array_equal(a['tree']['node_amaf'][r], b['tree']['node_amaf'][r]) for r in range(5))   # ... and its tree differs
    # a zero prior is the search without one
    z = me.tree_case(N, 0.0, 'zero', True)
    for k in ('parent', 'action', 'visits', 'node_amaf'):
        assert np.array_equal(z['tree'][k], plain['tree'][k]), k
    past = me.past_capacity_case()
    assert (past['nodes'][[0, 1, 2, 4]] == me.PAST_I + 1).all() and (past['root_visits'][[0, 1, 2, 4]] == (me.PAST_I + me.PAST_EXTRA) * me.TREE_K).all()
    assert math.isclose(me.TREE_FPU, 0.5)
