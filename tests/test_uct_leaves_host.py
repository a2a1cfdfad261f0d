"""CPU: the UCT search with several leaves per root and round (include/gymgo_amd_uct_leaves.h, gogame.batch_uct(leaves=L)) without a
device - the binding table of the family (_lib.ABI_UCT_LEAVES) against its header, the argument checks of the C entry points in
their order, every ValueError of the keyword before a device is touched, the launches the host loop queues, and the restatement
the GPU tests build on (tests/mc_uct_leaves_expect.py): L = 1 is the one-leaf restatement field for field, the invariants of
L > 1, and the premises of every case tests/test_gpu_uct_leaves.py runs."""
import ctypes
import math
import os

import numpy as np
import pytest

import mc_amaf_expect as ma
import mc_expect as mc
import mc_prior_expect as mq
import mc_uct_leaves_expect as ml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['gg_uct_select_leaves', 'gg_uct_backup_leaves', 'gg_uct_select_leaves_rave', 'gg_uct_backup_leaves_rave',
         'gg_uct_prior_expand_leaves']
HEADER = 'gymgo_amd_uct_leaves.h'


@pytest.fixture(scope='module')
def built(native_built):
    from gymgo_amd import _lib
    return _lib


# ---------------------------------------------------------------- the family's header against its binding table
def test_uct_leaves_binding_table_matches_its_header(native_built):
    import test_host_abi as tha
    from gymgo_amd import _lib
    decls = tha.header_declarations(HEADER)
    assert list(decls) == NAMES
    assert tha._abi_mismatches(decls, _lib.ABI_UCT_LEAVES) == []
    assert _lib.EXPORTS_UCT_LEAVES == tuple(decls)
    others = (_lib.EXPORTS, _lib.EXPORTS_AREA, _lib.EXPORTS_PAST, _lib.EXPORTS_GUMBEL, _lib.EXPORTS_TACTICS, _lib.EXPORTS_AMAF,
              _lib.EXPORTS_PATTERN, _lib.EXPORTS_PRIOR, _lib.EXPORTS_STATUS)
    assert not set(decls) & {f for t in others for f in t}                      # no name in common with the other tables
    assert all(_lib.ABI_ALL[f] is _lib.ABI_UCT_LEAVES[f] for f in NAMES)        # ... and merged into the one lookup
    dropped = dict(_lib.ABI_UCT_LEAVES, gg_uct_select_leaves=_lib.ABI_UCT_LEAVES['gg_uct_select_leaves'][1:])
    assert any('17 parameters in the header, 16 in the table' in b for b in tha._abi_mismatches(decls, dropped))   # the comparison can fail
    for f, (argtypes, restype) in _lib._SIGNATURES_UCT_LEAVES.items():          # the ctypes signatures come from the table
        assert restype is ctypes.c_int32
        assert argtypes == [p.kind if isinstance(p.kind, type) else ctypes.c_void_p for p in _lib.ABI_UCT_LEAVES[f]]
        assert _lib._POINTERS[f][0] == len(_lib.ABI_UCT_LEAVES[f])
    # each call is its namesake's list plus L behind I, and - select and backup - virt
    namesakes = {'gg_uct_select_leaves': _lib.ABI['gg_uct_select'], 'gg_uct_backup_leaves': _lib.ABI['gg_uct_backup'],
                 'gg_uct_select_leaves_rave': _lib.ABI_AMAF['gg_uct_select_rave'], 'gg_uct_backup_leaves_rave': _lib.ABI_AMAF['gg_uct_backup_rave'],
                 'gg_uct_prior_expand_leaves': _lib.ABI_PRIOR['gg_uct_prior_expand']}
    for f, base in namesakes.items():
        ps = _lib.ABI_UCT_LEAVES[f]
        names = [p.name for p in ps]
        assert names[names.index('I') + 1] == 'L' and ps[names.index('L')].kind is ctypes.c_int32
        assert tuple(p for p in ps if p.name not in ('L', 'virt')) == tuple(base), f
        assert ('virt' in names) == (f != 'gg_uct_prior_expand_leaves')
    hdr = open(os.path.join(ROOT, 'include', HEADER)).read()
    for word in ('Collision', 'virt int32 [R][C + 1]', 'r L + j', 'never below 0', 'GG_E_NULLPTR', 'first_root L'):
        assert word in hdr, word
    for doc in ('INTEGRATION.md', 'README.md'):
        text = open(os.path.join(ROOT, doc)).read()
        for name in NAMES + [HEADER]:
            assert name in text, (doc, name)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in decls:
        assert hasattr(L, name), name
    assert native_built.gg_version() == _lib.ABI_VERSION == 5                   # additive: the ABI version stays


# ---------------------------------------------------------------- the argument checks, in their order
def _select(L, rave=False, R=4, N=9, C=8, S=2, K=4, c=1.0, k=8.0, fpu=0.5, ptr=1, **null):
    p = lambda name: None if (not ptr or null.get(name)) else 1
    if rave:
        return L.gg_uct_select_leaves_rave(R, N, C, S, K, c, k, fpu, *[p(n) for n in ('log_table', 'boards', 'child', 'links', 'stats',
                                           'node_amaf', 'nodes', 'virt', 'leaf', 'move', 'leaf_id')], None)
    return L.gg_uct_select_leaves(R, N, C, S, K, c, *[p(n) for n in ('log_table', 'boards', 'child', 'links', 'stats', 'nodes', 'virt',
                                  'leaf', 'move', 'leaf_id')], None)


def _backup(L, rave=False, R=4, N=9, C=8, S=2, K=4, ptr=1, **null):
    p = lambda name: None if (not ptr or null.get(name)) else 1
    if rave:
        return L.gg_uct_backup_leaves_rave(R, N, C, S, K, *[p(n) for n in ('counts', 'sums', 'amaf', 'totals', 'boards', 'links', 'stats',
                                           'node_amaf', 'virt', 'leaf', 'move', 'leaf_id')], None)
    return L.gg_uct_backup_leaves(R, N, C, S, K, *[p(n) for n in ('counts', 'sums', 'totals', 'boards', 'links', 'stats', 'virt', 'leaf',
                                  'move', 'leaf_id')], None)


def test_entry_points_check_arguments_in_order(built):
    """Pointers that are never followed: every call below returns from its checks."""
    L = built.lib()
    for rave in (False, True):
        for fn in (_select, _backup):
            call = lambda **kw: fn(L, rave, **kw)
            assert call(N=1) == -1 and call(N=20) == -1 and call(R=-1) == -1
            assert call(C=0) == -3 and call(C=-2) == -3 and call(K=0) == -3
            assert call(S=0) == -3 and call(S=-1) == -3                         # L < 1
            assert call(N=20, S=0) == -1                                        # the sizes before the arguments
            assert call(C=2 ** 16, K=2 ** 15) == -1                             # the root's n = C K must fit an int32
            assert call(C=2 ** 16, K=2 ** 15, S=0) == -3                        # ... after the arguments
            assert call(R=2 ** 62, S=2) == -1 and call(R=2 ** 62, S=1, ptr=0) == -2     # R L rows are an int64
            assert call(ptr=0) == -2 and call(S=0, ptr=0) == -3                 # the pointers last
            assert call(R=0, ptr=0) == -2                                       # NULL buffers are an error even with nothing to do
            assert call(R=0) == 0
            assert call(virt=True) == -2                                        # virt is required
            if rave:
                assert call(C=2 ** 15, K=2 ** 15) == -1                         # 2 C K = 2^31
                assert call(C=2 ** 15 - 1, K=2 ** 15, ptr=0) == -2
                assert call(node_amaf=True) == -2
            else:
                assert call(C=2 ** 15, K=2 ** 15, ptr=0) == -2                  # C K = 2^30: allowed without RAVE
        for name in ('log_table', 'boards', 'child', 'links', 'stats', 'nodes', 'virt', 'leaf', 'move', 'leaf_id'):
            assert _select(L, rave, **{name: True}) == -2, name
        for name in ('counts', 'sums', 'boards', 'links', 'stats', 'virt', 'leaf', 'move', 'leaf_id') + (('amaf',) if rave else ()):
            assert _backup(L, rave, **{name: True}) == -2, name
        assert _backup(L, rave, totals=True, R=0) == 0                          # totals is the only optional buffer (R = 0: no launch)
        for c in (-1.0, -1e-300, math.inf, math.nan):
            assert _select(L, rave, c=c) == -3 and _select(L, rave, c=c, ptr=0) == -3
    for k in (0.0, -1.0, math.inf, math.nan):
        assert _select(L, True, k=k) == -3
    for fpu in (math.inf, -math.inf, math.nan):
        assert _select(L, True, fpu=fpu) == -3
    assert _select(L, True, k=0.0, C=2 ** 15, K=2 ** 15) == -1                 # the RAVE size before the RAVE arguments

    def expand(R=4, N=9, C=3, S=2, weights=16, leaf=16, move=16, leaf_id=16, amaf=16):
        return L.gg_uct_prior_expand_leaves(R, N, C, S, weights, leaf, move, leaf_id, amaf, None)

    assert expand(N=1) == -1 and expand(N=20) == -1 and expand(R=-1) == -1
    assert expand(C=0) == -3 and expand(C=2 ** 31 - 1) == -3 and expand(S=0) == -3 and expand(N=20, C=0) == -1
    assert expand(R=2 ** 62, S=2) == -1 and expand(R=2 ** 62, S=2, C=0) == -3
    for name in ('weights', 'leaf', 'move', 'leaf_id', 'amaf'):
        assert expand(**{name: None}) == -2 and expand(R=0, **{name: None}) == -2     # the pointers before "no work"
    assert expand(R=0) == 0 and expand(amaf=18) == -3 and expand(S=0, amaf=None) == -3


# ---------------------------------------------------------------- the Python API
def test_every_value_error_comes_before_a_device_is_touched():
    """On the parent commit `leaves=` is an unexpected keyword: TypeError, not ValueError."""
    from gymgo_amd import gogame
    st = np.zeros((2, 6, 5, 5), np.uint8)
    searches = ((gogame.batch_uct, st, 2), (gogame.uct_actions, st, 2), (gogame.uct, st[0], 1))
    for fn, s, R in searches:
        for bad in (0, -1, 1.5, '2', True, [2]):
            with pytest.raises(ValueError):
                fn(s, 4, 2, leaves=bad)
            with pytest.raises(ValueError):
                fn(s, 4, 2, leaves=bad, rave_equiv=8.0, prior=True)
        with pytest.raises(ValueError):
            fn(s, 1 << 10, 1 << 10, leaves=1 << 11)                             # T L K = 2^31
        with pytest.raises(ValueError):
            fn(s, 1 << 10, 1 << 10, leaves=1 << 10, rave_equiv=8.0)             # RAVE: 2 T L K = 2^31
        big = gogame.UctPrior((2 ** 29 - 5, 0), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0))
        with pytest.raises(ValueError):
            fn(s, 1 << 10, 1 << 10, leaves=1 << 9, rave_equiv=8.0, prior=big)   # the prior's bound counts T L K: 2 (2^29 + 2^29); UCT_PRIOR passes (below)
        with pytest.raises(ValueError):
            fn(s, 4, 2, leaves=2, policy='pattern', rave_equiv=8.0)             # as without leaves
        with pytest.raises(ValueError):
            fn(s, 4, 2, leaves=2, prior=True)                                   # a prior needs rave_equiv, as without leaves
    total = sum(v for v, _ in gogame.UCT_PRIOR)
    assert gogame._uct_prior_kw({'prior': True, 'rave_equiv': 1.0, 'leaves': 1 << 9}, lambda: (2, 5), 1 << 10, 1 << 10)[0] == gogame.UCT_PRIOR
    assert 2 * ((1 << 29) + total) < 2 ** 31
    assert gogame._uct_leaves(None) is None and gogame._uct_leaves(1) == 1 and gogame._uct_leaves(np.int32(64)) == 64
    doc = gogame.batch_uct.__doc__
    for word in ('leaves', 'virtual', 'collision', 'iterations * L + 1', '4 bytes a node', 'R * L rows', 'first_root * L'):
        assert word in doc or word.upper() in doc, word
    import torch
    if not torch.cuda.is_available():     # ... and there is no CPU path: what passes the checks ends at the device
        from gymgo_amd import _lib
        for kw in ({}, {'rave_equiv': 8.0}, {'rave_equiv': 8.0, 'prior': True}):
            with pytest.raises(_lib.GymGoNativeError):
                gogame.batch_uct(st, 4, 2, leaves=2, **kw)
        with pytest.raises(_lib.GymGoNativeError):
            gogame.uct(st[0], 4, 2, leaves=1)


def test_results_at_no_roots_and_the_launches_of_a_round(built, monkeypatch):
    """R = 0: no launch, results of the right shapes.  R > 0 with the device work stubbed out: the launches a search queues, in
    order - with leaves=None exactly the one-leaf entry points on R rows, with leaves=L the _leaves ones on R L rows."""
    import torch
    from gymgo_amd import gogame
    cpu = torch.device('cpu')
    monkeypatch.setattr(gogame, '_device', lambda: cpu)
    calls = []
    monkeypatch.setattr(built, 'call', lambda fn, *a: calls.append((fn,) + a))
    monkeypatch.setattr(built, 'current_raw_stream', lambda dev=None: 0)
    empty = np.zeros((0, 6, 5, 5), np.uint8)
    for kw, cls in (({}, gogame.Uct), ({'rave_equiv': 8.0}, gogame.UctRave), ({'rave_equiv': 8.0, 'prior': True}, gogame.UctRave)):
        res = gogame.batch_uct(empty, 3, 2, leaves=4, tree=True, slots=8, **kw)
        assert isinstance(res, cls) and res.visits.shape == (0, 26) and res.tree.parent.shape == (0, 13)
        assert 'rave_equiv' not in kw or res.tree.node_amaf.shape == (0, 13, 25, 2)
        assert gogame.batch_uct(empty, 3, 2, tree=True, slots=8, **kw).tree.parent.shape == (0, 4)
    assert calls == []
    played = []

    def run_playouts(roots, R, N, K, max_plies, komi, seed, first_root, ownership, S, chunk_plies, dev, buffers=None, policy=0, amaf=None):
        played.append((tuple(roots.shape), R, seed, first_root, tuple(buffers[5].shape), None if amaf is None else tuple(amaf[3].shape)))

    monkeypatch.setattr(gogame, '_run_playouts', run_playouts)
    R, N, T, K, L, W = 3, 5, 2, 2, 4, 26
    roots = torch.zeros((R, W), dtype=torch.int32)
    weights = torch.zeros(12, dtype=torch.int32)
    for rave, prior in ((None, None), ((8.0, 0.5), None), ((8.0, 0.5), (weights, None))):
        sfx = '' if rave is None else '_rave'
        for leaves in (None, 1, L):
            del calls[:], played[:]
            kw = {} if leaves is None else {'leaves': leaves}
            out = gogame._run_uct(roots, R, N, T, K, 0.5, 64, 0.5, 7, 5, 8, 32, cpu, 0, rave, prior, **kw)
            lf, rows, C = ('', R, T) if leaves is None else ('_leaves', R * leaves, T * leaves)
            one = ['gg_uct_select' + lf + sfx, 'gg_batch_play_moves_tracked'] + (['gg_uct_prior_expand' + lf] if prior else []) \
                + ['gg_uct_backup' + lf + sfx]
            assert [c[0] for c in calls] == ['gg_uct_begin'] + (['gg_uct_prior_begin'] if prior else []) + one * T
            assert out[0].shape == (R, C + 1, N * N + 1) and out[2].shape == (R, C + 1, 4)
            begin = calls[0]
            assert begin[2:6] == (R, N, C, K)
            sel = next(c for c in calls if c[0].startswith('gg_uct_select'))
            names = [p.name for p in built.ABI_ALL[sel[0]]]
            arg = lambda n: sel[1 + names.index(n)]
            assert len(sel) - 1 == len(names) and (arg('R'), arg('I')) == (R, C)
            assert arg('leaf').shape == (rows, W) and arg('move').shape == (rows,) and arg('log_table').shape == (C + 1,)
            if leaves is not None:
                assert arg('L') == leaves and arg('virt').shape == (R, C + 1) and not arg('virt').any()
            play = next(c for c in calls if c[0] == 'gg_batch_play_moves_tracked')
            assert play[4] == rows
            # the playouts: the rows as roots, first_root L, the round's seed, buffers for the rows
            fr = 5 * (leaves or 1)
            assert played == [((rows, W), rows, gogame._uct_seed(7, t), fr, (rows, 4), None if rave is None else (rows, 2, 3, N, N))
                              for t in range(T)]


# ---------------------------------------------------------------- L = 1 is the one-leaf search
def _host_roots(N):
    """The roots of tests/test_uct_host.py."""
    return np.concatenate([mc.make_roots(N, 3, 5, max_ply=N * N // 2, step=N)[1:2], mc.crafted_roots(N)])


def _same(a, b, root_keys, tree_keys, tag):
    for k in root_keys:
        assert np.array_equal(a[k], b[k]), (tag, k)
    for k in tree_keys:
        assert np.array_equal(a['tree'][k], b['tree'][k]), (tag, k)


@pytest.mark.parametrize('N,I,K', [(5, 40, 2), (9, 12, 3)])
def test_one_leaf_per_round_is_the_one_leaf_search(N, I, K):
    roots = _host_roots(N)
    kw = dict(c=0.8, komi=0.5, base_seed=4, first_root=2)
    one = ml.expected_uct_leaves(roots, I, 1, K, **kw)
    _same(mc.expected_uct(roots, I, K, **kw), one, mc.ROOT_KEYS, mc.TREE_KEYS, 'plain')
    assert all(t.collisions == 0 for t in one['trees']) and (one['live'] == 1).all()
    rave = ml.expected_uct_leaves(roots, I, 1, K, rave=(50.0, 0.5), **kw)
    _same(ma.expected_uct_rave(roots, I, K, rave_equiv=50.0, fpu=0.5, **kw), rave, ma.RAVE_ROOT_KEYS, ma.RAVE_TREE_KEYS, 'rave')
    last = np.array([N * N // 2, N * N, -1, 0, 3], np.int32)
    prior = ml.expected_uct_leaves(roots, I, 1, K, rave=(50.0, 0.5), prior=(mq.LOPSIDED, last), **kw)
    _same(mq.expected_uct_prior(roots, I, K, mq.LOPSIDED, last, rave_equiv=50.0, fpu=0.5, **kw), prior, ma.RAVE_ROOT_KEYS,
          ma.RAVE_TREE_KEYS + ('child',), 'prior')
    assert all(t.collisions == 0 for t in rave['trees'] + prior['trees'])


# ---------------------------------------------------------------- the invariants of L > 1
def _check_invariants(e, T, L, K, tag):
    for r, t in enumerate(e['trees']):
        used = len(t.boards)
        assert used == e['nodes'][r] and used <= T * L + 1, tag
        assert not t.v.any() and not t.boardless, tag                           # (asserted after every round by the restatement itself)
        own = np.zeros(T * L + 1, np.int64)
        for ev in t.log:
            assert len(ev) == L
            empty = [k == 'empty' for k, _, _ in ev]
            assert empty == sorted(empty), tag                                  # once a slot is empty, the later ones are
            for kind, _, y in ev:
                if y >= 0:
                    own[y] += 1
        assert e['root_visits'][r] == K * e['live'][:, r].sum() == K * own.sum(), tag
        n = t.stats[:, 0]
        for x in range(used):
            kids = t.child[x][t.child[x] >= 0]
            assert n[x] == K * own[x] + n[kids].sum(), (tag, x)                 # own evaluations + those through children
            assert t.stats[x, 1:].sum() == n[x], (tag, x)
        assert (e['tree']['visits'][r, used:] == 0).all() and (e['tree']['parent'][r, used:] == -1).all(), tag


@pytest.mark.parametrize('L', [2, 4, 8])
def test_invariants_of_several_leaves(L):
    for mode in ml.MODES:
        for N in (2, 5, 9):
            T, K, _, _ = ml.size_shape(N)
            _, e = ml.size_case(N, mode, L)
            _check_invariants(e, T, L, K, (mode, N, L))
        _, e = ml.ended_case(mode, L)
        _check_invariants(e, ml.ENDED_T, L, ml.ENDED_K, (mode, 'ended', L))
    # shards by root are the whole
    roots = ml.ended_roots()
    rave, prior = ml.mode_args('rave', 2, ml.ENDED_N)
    kw = dict(c=0.3, rave=rave, max_plies=64, komi=ml.KOMI, base_seed=77)
    whole = ml.ended_case('rave', L)[1]
    a = ml.expected_uct_leaves(roots[:1], ml.ENDED_T, L, ml.ENDED_K, **kw)
    b = ml.expected_uct_leaves(roots[1:], ml.ENDED_T, L, ml.ENDED_K, first_root=1, **kw)
    for k in ma.RAVE_ROOT_KEYS:
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k


def test_path_counts_between_select_and_backup():
    """v after a round's select is, node by node, the number of the round's leaves whose path goes through the node."""
    seen = []

    def look(t, trees):
        for tr in trees:
            want = np.zeros_like(tr.v)
            for _, _, y in tr.log[-1]:
                if y >= 0:
                    for z in tr.chain(y):
                        want[z] += 1
            assert np.array_equal(tr.v, want) and np.array_equal(tr.path_counts, want)
            seen.append(int(want[0]))

    roots = ml.ended_roots()
    ml.expected_uct_leaves(roots, 4, 4, 2, c=0.3, max_plies=64, base_seed=3, after_select=look)
    assert max(seen) == 4 and len(seen) == 8


# ---------------------------------------------------------------- the premises of tests/test_gpu_uct_leaves.py
def test_premises_of_the_device_cases():
    # collisions: at 2x2 and 3x3 with more slots than the root has legal actions, in every mode
    for N in (2, 3):
        for mode in ml.MODES:
            roots, e = ml.size_case(N, mode, 8)
            few = [r for r, root in enumerate(roots) if 0 < mc.legal_actions(root).size < 8]
            assert few and sum(e['trees'][r].collisions for r in few) > 0, (N, mode)
            assert (e['live'] < 8).any() and e['nodes'].max() <= ml.size_shape(N)[0] * 8 + 1
    # ... and with a large c in plain mode
    _, e = ml.c_case('plain', ml.BIG_C)
    assert sum(t.collisions for t in e['trees']) > 0
    # an ended node taken by two slots of one round, 5x5
    for mode in ('plain', 'prior'):
        _, e = ml.ended_case(mode, 8)
        assert sum(ml.ended_twice(t) for t in e['trees'][:1]) > 0, mode          # (below `passed`: not the root itself)
        assert any(k == 'ended' and d > 0 for t in e['trees'] for ev in t.log for k, d, _ in ev), mode
    # a round with both expanding (at the root) and descending slots, in every mode
    for mode in ml.MODES:
        both = 0
        for L in (2, 4, 8):
            _, e = ml.size_case(5, mode, L)
            both += sum(('expand', False) in ks and any(d for _, d in ks) for t in e['trees'] for ks in ml.kinds(t))
        assert both > 0, mode
    # under RAVE, a slot's choice differs from what v = 0 would have chosen
    for mode in ('rave', 'prior'):
        for N in (5, 9, 19):
            assert sum(t.vl_changed for L in ml.size_L(N, mode) for t in ml.size_case(N, mode, L)[1]['trees']) > 0, (mode, N)
    # every size runs every mode with every L
    cases = ml.all_size_cases()
    assert set(cases) == {(N, m, L) for N in ml.SIZES for m in ml.MODES for L in ml.LS} and len(cases) == 18 * 3 * 4
    for N in ml.SIZES:
        T, K, cap, names = ml.size_shape(N)
        assert 1 <= K <= 4 and T <= 6 and cap in (32, 64) and (N < 13 or len(names) <= 4)
    # the wide case fills its 64 slots at a root and stays inside its tree
    _, e = ml.wide_case('plain')
    assert e['live'].max() == 64 and e['nodes'].max() == 129
    # c = 0, sqrt 2 and 1e6 give different trees under RAVE
    trees = [ml.c_case('rave', c)[1]['tree']['parent'] for c in (0.0, math.sqrt(2), ml.BIG_C)]
    assert not np.array_equal(trees[0], trees[1])
