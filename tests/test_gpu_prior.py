"""-m gpu: the move priors on the device (include/gymgo_amd_prior.h) - the pairs of gg_batch_move_priors[_tracked] at
every board size against tests/mc_prior_expect.py and against the same combination of the planes of gg_batch_tactics and
gg_batch_patterns, later trips of the grid-stride loop, the RAVE search with priors bit for bit (child tables, links, stats, node
counts, AMAF pairs), a zero prior and no prior, independence from the playout queue, the four entry points between guards at
every start residue, and the forwarding calls.  tests/test_prior_host.py holds the cases to their premises on the CPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mc_amaf_expect as ma    # noqa: E402
import mc_expect as mc         # noqa: E402
import mc_prior_expect as me   # noqa: E402


def _stream():
    from gymgo_amd import _lib
    return _lib.stream_ptr(torch.device('cuda', torch.cuda.current_device()))


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _weights(w):
    return _i32([x for p in w for x in p])


# ---------------------------------------------------------------- the pairs
def _pairs_from_planes(dev, last, w):
    """The rule from the planes of gg_batch_tactics and gg_batch_patterns on the device -> int32 [B, N*N, 2]."""
    from gymgo_amd import gogame
    B, N = dev.shape[0], dev.shape[-1]
    t = gogame.batch_tactics(dev).to(torch.int32)
    p = gogame.batch_patterns(dev, last=last).to(torch.int32)
    ended = dev[:, 5].reshape(B, -1).any(dim=1)
    valid = ((dev[:, 3] == 0) & ~ended[:, None, None]).to(torch.int32)
    sets = (valid, t[:, 0], t[:, 1], p[:, 0] * valid, p[:, 1], valid * (1 - t[:, 2]))
    out = torch.zeros((B, N * N, 2), dtype=torch.int32, device=dev.device)
    for s, (v, x) in zip(sets, w):
        out[:, :, 0] += s.reshape(B, -1) * v
        out[:, :, 1] += s.reshape(B, -1) * (2 * x)
    return out


@pytest.mark.parametrize('N', me.SIZES)
def test_pairs_every_size(N):
    from gymgo_amd import gogame
    st, real = me.pair_boards(N)
    B = len(st)
    dev = mc.to_dev(st)
    tr = gogame.batch_track(dev)
    for tag, last in me.last_variants(N, B, real):
        for w in (me.DEFAULT, me.LOPSIDED):
            want = me.prior_pairs(st, last, w).astype(np.int32)
            got = gogame.batch_move_priors(dev, gogame.UctPrior(*w), last=last)
            assert got.dtype == torch.int32 and tuple(got.shape) == (B, N * N, 2)
            bad = np.flatnonzero((got.cpu().numpy() != want).reshape(B, -1).any(axis=1))
            assert len(bad) == 0, (N, tag, bad[:8].tolist())
            assert torch.equal(got, _pairs_from_planes(dev, last, w)), (N, tag, 'planes')
            assert torch.equal(got, gogame.batch_move_priors_tracked(tr, gogame.UctPrior(*w), last=last)), (N, tag, 'tracked')
    assert torch.equal(gogame.batch_move_priors(dev), gogame.batch_move_priors(dev, gogame.UCT_PRIOR, last=None))     # prior=True: the default
    assert bool((dev == mc.to_dev(st)).all())
    if N == 4:      # NumPy in, NumPy out; the single-state form; an empty batch
        got = gogame.batch_move_priors(np.array(st), True, last=real)
        assert isinstance(got, np.ndarray) and np.array_equal(got, me.prior_pairs(st, real, me.DEFAULT))
        k = int(np.flatnonzero((real >= 0) & (real < N * N))[0])
        assert np.array_equal(gogame.move_priors(st[k], me.LOPSIDED, last=int(real[k])), me.prior_pairs(st[k:k + 1], real[k:k + 1], me.LOPSIDED)[0])
        assert tuple(gogame.batch_move_priors(dev[:0]).shape) == (0, N * N, 2)


TRIPS = r'''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
from gymgo_amd import _lib, gogame
import mc_expect as mc
import mc_prior_expect as me
assert _lib.lib().gg_device_cus() == 1
# one compute unit: a grid of 64 single-wave workgroups.  533 boards are 134 groups of four (N <= 13: three trips, the last group
# one board) or 267 groups of two (19x19: five trips); a chunk of 61 boards stays below the cap
B, CH = 533, 61
for N in (5, 9, 13, 19):
    st0, la0 = me.pair_boards(N)
    i = (5 * np.arange(B)) %% len(st0)
    st, last = st0[i], la0[i]
    dev, la = mc.to_dev(st), torch.from_numpy(last.copy()).cuda()
    tr = gogame.batch_track(dev)
    whole = gogame.batch_move_priors(dev, True, last=la)
    parts = torch.cat([gogame.batch_move_priors(dev[b:b + CH], True, last=la[b:b + CH]) for b in range(0, B, CH)])
    assert torch.equal(whole, parts), (N, 'bytes')
    assert torch.equal(gogame.batch_move_priors_tracked(tr, True, last=la), parts), (N, 'tracked')
    assert np.array_equal(whole.cpu().numpy(), me.prior_pairs(st, last, me.DEFAULT)), (N, 'expected')
    # ... and into the trees of 533 roots: node 0 gets the pairs on top of what is there, node 1 keeps its words
    w = torch.tensor([x for p in me.DEFAULT for x in p], dtype=torch.int32).cuda()
    amaf = torch.arange(B * 2 * N * N * 2, dtype=torch.int32, device='cuda').reshape(B, 2, N * N, 2) %% 1000
    base = amaf.clone()
    _lib.call('gg_uct_prior_begin', tr, la, B, N, 1, w, amaf, _lib.stream_ptr(dev.device))
    assert torch.equal(amaf[:, 0] - base[:, 0], parts) and torch.equal(amaf[:, 1], base[:, 1]), (N, 'tree')
torch.cuda.synchronize()
print('PRIOR TRIPS OK')
''' % (ROOT, os.path.join(ROOT, 'tests'))


def test_later_trips_of_the_grid_stride_loop():
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '1'
    p = subprocess.run([sys.executable, '-c', TRIPS], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'PRIOR TRIPS OK' in p.stdout


# ---------------------------------------------------------------- the search
def _search(N, c, w, last, I=me.TREE_I, iterations=None, seed=None, S=7, chunk=32):
    """The RAVE search with priors through the entry points, as gogame._run_uct queues it -> dict of NumPy arrays: child, links,
    stats, nodes, totals, node_amaf.  iterations: how many to run on trees of I + 1 nodes (default I, through _run_uct itself)."""
    from gymgo_amd import _lib, gogame
    roots, _ = me.tree_roots(N)
    R, K = len(roots), me.TREE_K
    dev = mc.to_dev(roots)
    tr = gogame.batch_track(dev)
    cap = ma.cs.full_cap(N, chunk)
    seed = me.tree_seed(N) if seed is None else seed
    prior = None if w is None else (_weights(w), None if last is None else _i32(last))
    if iterations is None:
        child, links, stats, nodes, totals, node_amaf = gogame._run_uct(tr, R, N, I, K, c, cap, me.TREE_KOMI, seed, 0, S, chunk, dev.device,
                                                                        rave=(me.TREE_EQUIV, me.TREE_FPU), prior=prior)
    else:
        W, A, NN = 5 * N + 1, N * N + 1, I + 1
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device='cuda')
        boards, child, links, stats, nodes = i32(R, NN, W), i32(R, NN, A), i32(R, NN, 2), i32(R, NN, 4), i32(R)
        leaf, move, leaf_id = i32(R, W), i32(R), i32(R)
        totals = torch.zeros((R, 2), dtype=torch.int64, device='cuda')
        node_amaf = torch.zeros((R, NN, N * N, 2), dtype=torch.int32, device='cuda')
        L = torch.from_numpy(mc.log_table(I, K)).cuda()
        pbufs, abufs = gogame._playout_buffers(R, S, N, 'cuda'), gogame._amaf_buffers(R, S, N, chunk, 'cuda')
        s = _stream()
        _lib.call('gg_uct_begin', tr, R, N, I, K, boards, child, links, stats, nodes, s)
        _lib.call('gg_uct_prior_begin', tr, prior[1], R, N, I, prior[0], node_amaf, s)
        for i in range(iterations):
            _lib.call('gg_uct_select_rave', R, N, I, K, c, me.TREE_EQUIV, me.TREE_FPU, L, boards, child, links, stats, node_amaf, nodes, leaf,
                      move, leaf_id, s)
            _lib.call('gg_batch_play_moves_tracked', leaf, move, None, R, N, 1, s)
            _lib.call('gg_uct_prior_expand', R, N, I, prior[0], leaf, move, leaf_id, node_amaf, s)
            gogame._run_playouts(leaf, R, N, K, cap, me.TREE_KOMI, gogame._uct_seed(seed, i), 0, False, S, chunk, torch.device('cuda', 0), pbufs,
                                 0, amaf=abufs)
            _lib.call('gg_uct_backup_rave', R, N, I, K, pbufs[5], pbufs[6], abufs[3], totals, boards, links, stats, node_amaf, leaf, move,
                      leaf_id, s)
    assert bool((dev == mc.to_dev(roots)).all())
    return {k: v.cpu().numpy() for k, v in (('child', child), ('links', links), ('stats', stats), ('nodes', nodes), ('totals', totals),
                                            ('node_amaf', node_amaf))}


def _check_tree(got, want, tag):
    t = want['tree']
    for k, w in (('nodes', want['nodes']), ('child', t['child']), ('links', np.stack([t['parent'], t['action']], axis=-1)),
                 ('stats', np.stack([t[k] for k in ('visits', 'black_wins', 'white_wins', 'draws')], axis=-1)), ('node_amaf', t['node_amaf']),
                 ('totals', np.stack([want['unfinished'], want['plies_sum']], axis=-1))):
        assert got[k].shape == w.shape, (tag, k, got[k].shape, w.shape)
        assert np.array_equal(got[k], w), (tag, k, np.argwhere(got[k] != w)[:6].tolist())


@pytest.mark.parametrize('with_last', (False, True))
@pytest.mark.parametrize('prior', ('default', 'lopsided'))
@pytest.mark.parametrize('c', me.TREE_CS)
@pytest.mark.parametrize('N', me.TREE_SIZES)
def test_uct_prior_whole_tree(N, c, prior, with_last):
    _, last = me.tree_roots(N)
    want = me.tree_case(N, c, prior, with_last)
    got = _search(N, c, me.PRIORS[prior], last if with_last else None)
    _check_tree(got, want, (N, c, prior, with_last))


def test_uct_prior_past_capacity():
    """PAST_I + PAST_EXTRA iterations on trees with room for PAST_I + 1 nodes: once a tree is full nothing is expanded - move is -1
    and gg_uct_prior_expand leaves every pair as it is."""
    _, last = me.tree_roots(me.PAST_N)
    got = _search(me.PAST_N, 0.5, me.DEFAULT, last, I=me.PAST_I, iterations=me.PAST_I + me.PAST_EXTRA, seed=31, S=6)
    _check_tree(got, me.past_capacity_case(), 'past capacity')


def _uct(N, dev, **kw):
    from gymgo_amd import gogame
    return gogame.batch_uct(dev, me.TREE_I, me.TREE_K, komi=me.TREE_KOMI, seed=me.tree_seed(N), tree=True, rave_equiv=me.TREE_EQUIV,
                            fpu=me.TREE_FPU, **kw)


def _same_result(a, b, tag):
    assert type(a) is type(b) and type(a.tree) is type(b.tree), tag
    for k in ma.RAVE_ROOT_KEYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), (tag, k)
    for k in ma.RAVE_TREE_KEYS:
        assert torch.equal(getattr(a.tree, k), getattr(b.tree, k)), (tag, k)


@pytest.mark.parametrize('N', (2, 9, 19))
def test_a_zero_prior_and_no_prior_are_the_search_without_one(N):
    from gymgo_amd import gogame
    roots, last = me.tree_roots(N)
    dev = mc.to_dev(roots)
    plain = _uct(N, dev, c=0.7)
    assert type(plain) is gogame.UctRave
    _same_result(_uct(N, dev, c=0.7, prior=None), plain, (N, 'none'))
    _same_result(_uct(N, dev, c=0.7, prior=gogame.UctPrior(*me.ZERO)), plain, (N, 'zero'))
    _same_result(_uct(N, dev, c=0.7, prior=gogame.UctPrior(*me.ZERO), last_actions=last), plain, (N, 'zero, last'))
    seeded = _uct(N, dev, c=0.7, prior=True)
    assert not torch.equal(seeded.rave_visits, plain.rave_visits)


@pytest.mark.parametrize('N', (5, 19))
def test_python_api_queue_independence_and_shards(N):
    """batch_uct itself against the expectation - the result's rave_visits / rave_score include the root's prior -, whatever the
    slots and chunk_plies of the playout queue; shards by first_root concatenate to the whole."""
    from gymgo_amd import gogame
    roots, last = me.tree_roots(N)
    dev = mc.to_dev(roots)
    c = math.sqrt(2)
    want = me.tree_case(N, c, 'default', True)
    keys = ma.RAVE_ROOT_KEYS
    for slots, chunk in ((None, 32), (3, 8), (11, 16)):
        got = _uct(N, dev, c=c, prior=True, last_actions=last, slots=slots, chunk_plies=chunk, max_plies=ma.cs.full_cap(N))
        assert type(got) is gogame.UctRave and type(got.tree) is gogame.UctRaveTree
        mc.check(got, want, keys, (N, slots, chunk))
        mc.check(got.tree, want['tree'], ma.RAVE_TREE_KEYS, (N, slots, chunk))
    root_prior = me.prior_pairs(roots, last, me.DEFAULT)
    assert (want['rave_visits'] >= root_prior[:, :, 0]).all() and root_prior.any()
    a = _uct(N, dev[:2], c=c, prior=True, last_actions=last[:2])
    b = _uct(N, dev[2:], c=c, prior=gogame.UCT_PRIOR, last_actions=torch.from_numpy(last[2:].copy()), first_root=2, slots=5)
    for k in keys:
        assert np.array_equal(np.concatenate([mc.to_np(getattr(a, k)), mc.to_np(getattr(b, k))]), want[k]), (N, k)
    for k in ma.RAVE_TREE_KEYS:
        assert np.array_equal(np.concatenate([mc.to_np(getattr(a.tree, k)), mc.to_np(getattr(b.tree, k))]), want['tree'][k]), (N, k)


def test_forwarding_calls_agree_with_batch_uct():
    from gymgo_amd import gogame
    N = 5
    roots, last = me.tree_roots(N)
    dev = mc.to_dev(roots)
    kw = dict(c=0.0, komi=me.TREE_KOMI, seed=me.tree_seed(N), rave_equiv=me.TREE_EQUIV, fpu=me.TREE_FPU)
    want = me.tree_case(N, 0.0, 'default', True)
    acts = gogame.uct_actions(dev, me.TREE_I, me.TREE_K, prior=True, last_actions=last, slots=5, chunk_plies=16, **kw)
    assert np.array_equal(mc.to_np(acts), mc.most_visited(want))
    assert np.array_equal(gogame.uct_actions(np.array(roots), me.TREE_I, me.TREE_K, prior=True, last_actions=list(last), **kw), mc.most_visited(want))
    for r in (1, 4):
        one = gogame.uct(dev[r], me.TREE_I, me.TREE_K, prior=gogame.UCT_PRIOR, last_actions=int(last[r]), first_root=r, tree=True, **kw)
        assert type(one) is gogame.UctRave
        for k in ma.RAVE_ROOT_KEYS:
            assert np.array_equal(mc.to_np(getattr(one, k)), want[k][r]), (r, k)
        assert np.array_equal(mc.to_np(one.tree.node_amaf), want['tree']['node_amaf'][r]), r
    no_last = gogame.uct_actions(dev, me.TREE_I, me.TREE_K, prior=True, **kw)
    assert np.array_equal(mc.to_np(no_last), mc.most_visited(me.tree_case(N, 0.0, 'default', False)))


# ---------------------------------------------------------------- guards
def _arena_views(specs, k, device='cuda'):
    """An arena with one view per (name, shape, dtype, readonly) of specs, buffer j at the (k + j)-th residue its element size allows."""
    import guard_arena as ga
    arena = ga.Arena(sum(ga.footprint(shape, dtype) for _, shape, dtype, _ in specs) + 64, device)
    views = {}
    for j, (name, shape, dtype, ro) in enumerate(specs):
        res = ga.residues(dtype)
        views[name] = arena.take(name, shape, dtype, res[(k + j) % len(res)], readonly=ro)
    return arena, views


GUARD_SIZES = (2, 9, 13, 19)
GUARD_B = 7          # a full wave of boards and a ragged one, at four and at two boards per wave


def _guard_boards(N):
    """GUARD_B boards of pair_boards(N) with their previous actions: boards with a local answer first, then others whose previous
    action is a point, a finished game, and board 0 (no previous point)."""
    st0, la0 = me.pair_boards(N)
    local = me.prior_sets(st0, la0)[4].reshape(len(st0), -1).any(axis=1)
    real = (la0 >= 0) & (la0 < N * N)
    pick = (np.flatnonzero(local)[:3].tolist() + np.flatnonzero(real & ~local).tolist())[:GUARD_B - 2]
    pick += [int(np.flatnonzero(st0[:, 5, 0, 0] != 0)[0]), 0]
    assert len(pick) == GUARD_B and local[pick].any()
    return st0[pick], la0[pick]


@pytest.mark.parametrize('N', GUARD_SIZES)
def test_guards_batch_move_priors(N):
    from gymgo_amd import _lib, gogame
    st, last = _guard_boards(N)
    B, P, W = len(st), N * N, 5 * N + 1
    want = me.prior_pairs(st, last, me.LOPSIDED).astype(np.int32)
    assert want.any()
    dev = mc.to_dev(st)
    tr0 = gogame.batch_track(dev)
    i32 = torch.int32
    for k in range(16):
        for name, boards, shape, dt in (('gg_batch_move_priors', dev, (B, 6, N, N), torch.uint8), ('gg_batch_move_priors_tracked', tr0, (B, W), i32)):
            arena, v = _arena_views([('boards', shape, dt, True), ('last', (B,), i32, True), ('weights', (12,), i32, True),
                                     ('out', (B, P, 2), i32, False)], k)
            v['boards'].copy_(boards)
            v['last'].copy_(_i32(last))
            v['weights'].copy_(_weights(me.LOPSIDED))
            arena.snapshot()
            _lib.call(name, v['boards'], v['last'], v['weights'], v['out'], B, N, _stream())
            assert arena.violations() == [], (N, k, name)
            assert np.array_equal(v['out'].cpu().numpy(), want), (N, k, name)
            arena.refill('out')
            arena.snapshot()
            _lib.call(name, v['boards'], None, v['weights'], v['out'], B, N, _stream())           # last = NULL
            assert arena.violations() == [], (N, k, name, 'no last')
            assert np.array_equal(v['out'].cpu().numpy(), me.prior_pairs(st, None, me.LOPSIDED)), (N, k, name, 'no last')


@pytest.mark.parametrize('N', GUARD_SIZES)
def test_guards_uct_prior_begin_and_expand(N):
    """Both tree calls ADD: node_amaf starts from known words, the named node of every root gains the pairs, every other word of the
    buffer and every byte around it stays.  expand skips a root whose move is -1 and one whose leaf_id is outside [0, I]."""
    from gymgo_amd import _lib, gogame
    st, last = _guard_boards(N)
    R, P, W, I = len(st), N * N, 5 * N + 1, 3
    pairs = me.prior_pairs(st, last, me.DEFAULT).astype(np.int32)
    plain_pairs = me.prior_pairs(st, None, me.DEFAULT).astype(np.int32)
    assert pairs.any() and not np.array_equal(pairs, plain_pairs)
    tr0 = gogame.batch_track(mc.to_dev(st))
    base = (np.arange(R * (I + 1) * P * 2, dtype=np.int64) * 7 % 1013).astype(np.int32).reshape(R, I + 1, P, 2)
    # expand: the previous action is the move - a point for the first roots, then the pass, -1 (skipped); leaf ids over the tree,
    # two of them outside it (skipped)
    move = last.copy()
    move[-1], move[-2] = -1, P
    leaf_id = np.array([(3 * r + 1) % (I + 1) for r in range(R)], np.int32)
    leaf_id[1], leaf_id[2] = -1, I + 1
    exp_pairs = me.prior_pairs(st, move, me.DEFAULT).astype(np.int32)
    want_expand = base.copy()
    for r in range(R):
        if move[r] >= 0 and 0 <= leaf_id[r] <= I:
            want_expand[r, leaf_id[r]] += exp_pairs[r]
    changed = (want_expand != base).reshape(R, -1).any(axis=1)
    assert changed.sum() >= 3 and not changed[[1, 2, R - 1]].any()
    i32 = torch.int32
    for k in range(16):
        arena, v = _arena_views([('roots', (R, W), i32, True), ('last_actions', (R,), i32, True), ('weights', (12,), i32, True),
                                 ('node_amaf', (R, I + 1, P, 2), i32, False)], k)
        v['roots'].copy_(tr0)
        v['last_actions'].copy_(_i32(last))
        v['weights'].copy_(_weights(me.DEFAULT))
        for la, want in ((v['last_actions'], pairs), (None, plain_pairs)):
            v['node_amaf'].copy_(_i32(base))
            arena.snapshot()
            _lib.call('gg_uct_prior_begin', v['roots'], la, R, N, I, v['weights'], v['node_amaf'], _stream())
            assert arena.violations() == [], (N, k, 'begin')
            got = v['node_amaf'].cpu().numpy()
            assert np.array_equal(got[:, 0] - base[:, 0], want) and np.array_equal(got[:, 1:], base[:, 1:]), (N, k, 'begin')
        arena, v = _arena_views([('weights', (12,), i32, True), ('leaf', (R, W), i32, True), ('move', (R,), i32, True),
                                 ('leaf_id', (R,), i32, True), ('node_amaf', (R, I + 1, P, 2), i32, False)], k)
        v['leaf'].copy_(tr0)
        v['move'].copy_(_i32(move))
        v['leaf_id'].copy_(_i32(leaf_id))
        v['weights'].copy_(_weights(me.DEFAULT))
        v['node_amaf'].copy_(_i32(base))
        arena.snapshot()
        _lib.call('gg_uct_prior_expand', R, N, I, v['weights'], v['leaf'], v['move'], v['leaf_id'], v['node_amaf'], _stream())
        assert arena.violations() == [], (N, k, 'expand')
        assert np.array_equal(v['node_amaf'].cpu().numpy(), want_expand), (N, k, 'expand')
