"""CPU: PUCT self-play (gg_puct_root_noise / gg_puct_root_policy, gogame.PuctSearch.add_root_noise / root_policy,
dirichlet_noise, puct_selfplay) without a device - the argument checks of the C-ABI in their stated order, the ValueError
cases of the Python layer and their order, R = 0 and moves = 0, and the restatement the GPU tests build on
(tests/mc_puct_selfplay_expect.py): without sampling the move is most_visited_root's, a draw returns only legal visited
actions and its frequencies over 4 096 generator states follow n_a / S, the todo protocol reaches kept roots before round 0,
fresh roots after it and ended roots never, noise given twice changes a root once, pi rows sum to 1 or are all zero, and the
outcome is terminal_value's sign."""
import math

import numpy as np
import pytest

import mc_expect as mc
import mc_puct_expect as pe
import mc_puct_advance_expect as pa
import mc_puct_selfplay_expect as ps


@pytest.fixture(scope='module')
def built(native_built):
    from gymgo_amd import _lib
    return _lib


def _noise(L, R=4, N=9, C=8, eps=0.25, ptrs=None):
    p = [1] * 6 if ptrs is None else ptrs
    return L.gg_puct_root_noise(R, N, C, eps, p[0], p[1], p[2], p[3], p[4], p[5], None)


def _policy(L, R=4, N=9, C=8, ptrs=None, sample=None, rng=None, pi=1, value=1):
    p = [1] * 5 if ptrs is None else ptrs
    return L.gg_puct_root_policy(R, N, C, sample, rng, p[0], p[1], p[2], p[3], p[4], pi or None, value or None, None)


def test_entry_points_check_arguments_before_device_work(built):
    L = built.lib()
    for call, n in ((_noise, 6), (_policy, 5)):
        none = [None] * n
        assert call(L, N=1) == -1 and call(L, N=20) == -1 and call(L, R=-1) == -1
        assert call(L, C=0) == -3 and call(L, C=-2) == -3 and call(L, C=2 ** 31 - 1) == -3
        assert call(L, N=1, C=0, ptrs=none) == -1 and call(L, C=0, ptrs=none) == -3     # sizes, arguments, pointers
        assert call(L, R=0, C=0, ptrs=none) == -3                                       # ... also with nothing to do
        assert call(L, ptrs=none) == -2 and call(L, C=2 ** 31 - 2, ptrs=none) == -2
        assert call(L, R=0, ptrs=none) == 0 and call(L, R=0) == 0                       # R = 0 returns before any pointer check
        for i in range(n):                                                              # every buffer is required
            ptrs = [1] * n
            ptrs[i] = None
            assert call(L, ptrs=ptrs) == -2, (call.__name__, i)
    for eps in (-0.001, 1.001, math.nan, math.inf, -math.inf):
        assert _noise(L, eps=eps) == -3 and _noise(L, eps=eps, ptrs=[None] * 6) == -3 and _noise(L, R=0, eps=eps) == -3
    assert _noise(L, eps=0.0, ptrs=[None] * 6) == -2 and _noise(L, eps=1.0, ptrs=[None] * 6) == -2
    assert _policy(L, sample=1, rng=None) == -2                                         # sample needs rng
    assert _policy(L, R=0, sample=1, rng=None) == 0
    assert _policy(L, R=0, sample=None, rng=None, pi=0, value=0) == 0
    assert {'gg_puct_root_noise', 'gg_puct_root_policy'} <= set(built.EXPORTS)
    assert L.gg_version() == 5


def test_python_errors_their_order_and_empty_batches(built, monkeypatch):
    import torch
    from gymgo_amd import gogame
    monkeypatch.setattr(gogame, '_device', lambda: torch.device('cpu'))
    empty = np.zeros((0, 6, 5, 5), np.uint8)
    A = 26
    p, v = np.zeros((0, A), np.float32), np.zeros(0, np.float32)
    z, rng = np.zeros((0, A), np.float32), torch.zeros(0, dtype=torch.int64)
    s = gogame.PuctSearch(empty, 2, capacity=9)
    todo = s.add_root_noise(z)                                # before the first round: allowed
    assert isinstance(todo, torch.Tensor) and todo.dtype == torch.uint8 and tuple(todo.shape) == (0,)
    mine = torch.zeros(0, dtype=torch.bool)
    assert s.add_root_noise(torch.from_numpy(z), 0.0, mine) is mine and s.add_root_noise(z, 1, todo) is todo
    with pytest.raises(ValueError, match='eps'):
        s.add_root_noise(np.zeros((1, A), np.float32), eps=1.5)            # eps before the noise's shape
    with pytest.raises(ValueError, match='eps'):
        s.add_root_noise(z, eps=math.nan)
    with pytest.raises(ValueError, match='noise must be'):
        s.add_root_noise(np.zeros((0, A + 1), np.float32), todo=np.zeros(0, np.uint8))   # the noise before todo
    for bad in (np.zeros(0, np.uint8), torch.zeros(0, dtype=torch.int32), torch.zeros(1, dtype=torch.uint8), torch.zeros((0, 1), dtype=torch.bool)):
        with pytest.raises(ValueError, match='todo'):
            s.add_root_noise(z, todo=bad)
    acts, pi, val = s.root_policy()
    assert isinstance(acts, np.ndarray) and acts.dtype == np.int64 and acts.shape == (0,)
    assert pi.dtype == np.float32 and pi.shape == (0, A) and val.dtype == np.float32 and val.shape == (0,)
    assert s.root_policy(pi=False)[1] is None
    assert s.root_policy(sample=np.zeros(0, bool), rng=rng)[0].shape == (0,)
    with pytest.raises(ValueError, match='needs rng'):
        s.root_policy(sample=np.zeros(3, np.float32))                       # the missing rng before the sample's shape
    for bad in (np.zeros(1, bool), np.zeros(0, np.int32), np.zeros((0, 1), np.uint8)):
        with pytest.raises(ValueError, match='sample must be'):
            s.root_policy(sample=bad, rng=torch.zeros(1, dtype=torch.int32))   # the sample before the rng
    for bad in (np.zeros(0, np.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(1, dtype=torch.int64)):
        with pytest.raises(ValueError, match='rng must be'):
            s.root_policy(sample=np.zeros(0, np.uint8), rng=bad)
    s.select()
    with pytest.raises(ValueError, match='backed up'):
        s.add_root_noise(z, eps=7.0)                          # a select is outstanding: before every other check
    with pytest.raises(ValueError, match='backed up'):
        s.root_policy(sample=np.zeros(0, bool))
    s.backup(p, v)
    s.add_root_noise(z, todo=todo)
    s.root_policy()
    # puct_selfplay: the komi guard, moves, sample_moves, eps, noise, the states, the search's own arguments - in this order
    calls = []

    def ev(states, legal):
        calls.append((tuple(states.shape), tuple(legal.shape)))
        return p, v

    ev.komi = 7.5
    with pytest.raises(ValueError, match='komi'):
        gogame.puct_selfplay(empty, -1, 2, ev, komi=0.5)
    ev.komi = None
    kw = dict(moves=-1, sample_moves=-1, eps=2.0, noise=3, iterations=0)
    for name, match in (('moves', 'moves >= 0'), ('sample_moves', 'sample_moves'), ('eps', 'eps'), ('noise', 'noise must be')):
        with pytest.raises(ValueError, match=match):
            gogame.puct_selfplay(np.zeros((0, 5, 5, 5), np.uint8), kw['moves'], kw['iterations'], ev, sample_moves=kw['sample_moves'],
                                 eps=kw['eps'], noise=kw['noise'])
        kw[name] = {'moves': 3, 'sample_moves': 1, 'eps': 0.25, 'noise': None}[name]
    with pytest.raises(ValueError, match='batch_states'):
        gogame.puct_selfplay(np.zeros((0, 5, 5, 5), np.uint8), 3, 0, ev)
    for bad in (dict(iterations=0), dict(iterations=2, c=-1.0), dict(iterations=2, komi=math.inf), dict(iterations=2, leaves=0),
                dict(iterations=2, leaves=2, capacity=4)):
        for moves in (0, 3):
            with pytest.raises(ValueError):
                gogame.puct_selfplay(empty, moves, evaluator=ev, **bad)
    assert not calls
    # R = 0 and moves = 0: empty records of the right shapes, the evaluator is not called
    live = np.zeros((3, 6, 5, 5), np.uint8)
    for states, moves, R in ((empty, 4, 0), (empty, 0, 0), (live, 0, 3)):
        for rec in (False, True):
            got = gogame.puct_selfplay(states, moves, 2, ev, leaves=2, capacity=30, noise=lambda mv, legal: z, sample_moves=2,
                                       record_states=rec)
            assert isinstance(got, gogame.SelfPlay) and all(isinstance(x, np.ndarray) for x in got if x is not None)
            assert got.actions.shape == (R, moves) and got.actions.dtype == np.int64
            assert got.pi.shape == (R, moves, A) and got.pi.dtype == np.float32
            assert got.value.shape == (R, moves) and got.value.dtype == np.float32
            assert got.outcome.shape == (R,) and got.outcome.dtype == np.int8 and not got.outcome.any()
            assert got.lengths.shape == (R,) and got.lengths.dtype == np.int32 and not got.lengths.any()
            assert got.final_states.dtype == np.uint8 and np.array_equal(got.final_states, states)
            assert (got.states is None) if not rec else (got.states.shape == (R, moves, 6, 5, 5) and got.states.dtype == np.uint8)
    assert not calls
    for bad in (0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            gogame.dirichlet_noise(bad)
    row = gogame.dirichlet_noise(0.3, generator=torch.Generator().manual_seed(5))(0, torch.tensor([[True, False, True, True],
                                                                                                  [False] * 4]))
    assert row.dtype == torch.float32 and tuple(row.shape) == (2, 4) and abs(float(row[0].sum()) - 1) < 1e-6
    assert float(row[0, 1]) == 0 and not row[1].any() and bool((row >= 0).all())


def _searched(N=5, T=40, L=None, c=0.6, komi=0.5, evaluator=pe.hash_evaluator_np):
    roots = np.concatenate([mc.crafted_roots(N), mc.make_roots(N, 3, 9, max_ply=20, step=10)[1:2]])
    trees = pa.make_trees(roots, 3 * T * (L or 1) + 1, L)
    pa.search_rounds(trees, T, L, evaluator, c, komi)
    return roots, trees


@pytest.mark.parametrize('L', [None, 4])
def test_root_policy_on_the_restatement(L):
    roots, trees = _searched(L=L)
    A = roots.shape[-1] ** 2 + 1
    rng = ps.seeds(len(trees), 7)
    ended = 0
    for r, t in enumerate(trees):
        a, pi, value, x = ps.root_policy(t, 0, rng[r])
        assert a == pa.most_visited_root(t) and x == rng[r]                 # sample = 0: the most visits, no draw
        assert pi.dtype == np.float32 and pi.shape == (A,) and np.float32(value).dtype == np.float32
        n = ps.root_visits(t)
        if t.legal[0].size == 0:
            ended += 1
            assert a == -1 and not pi.any() and value == 0 and ps.root_policy(t, 1, rng[r])[3] == rng[r]
            continue
        assert abs(float(pi.astype(np.float64).sum()) - 1) < 1e-6 and n.sum() == t.n[0] - 1
        assert not pi[np.setdiff1d(np.arange(A), t.legal[0])].any() and np.array_equal(pi > 0, n > 0)
        s = -1.0 if t.boards[0][2, 0, 0] else 1.0
        assert value == np.float32(s * t.w[0] / t.n[0]) and -1 <= value <= 1
        x = rng[r]
        for _ in range(64):                                                 # a draw: legal, visited, the generator moves on
            a, pi2, value2, x2 = ps.root_policy(t, 1, x)
            assert a in t.legal[0] and n[a] > 0 and x2 == (x + mc.GOLDEN_GAMMA) % 2 ** 64
            assert np.array_equal(pe.bits(pi2), pe.bits(pi)) and value2 == value
            x = x2
    assert ended
    fresh = pa.make_trees(roots, 9, L)
    for r, t in enumerate(fresh):                                           # nothing searched: S = 0, all-zero rows, no draw
        a, pi, value, x = ps.root_policy(t, 1, rng[r])
        assert not pi.any() and value == 0 and x == rng[r] and a == (t.legal[0][0] if t.legal[0].size else -1)


def test_draw_frequencies_follow_the_visit_counts():
    _, trees = _searched(T=200, c=2.0)
    t = trees[0]                                                            # the empty board
    n = ps.root_visits(t)
    S = int(n.sum())
    assert (n > 0).sum() >= 3 and S == t.n[0] - 1
    draws = 4096
    seen = np.zeros(n.shape[0], np.int64)
    for x in ps.seeds(draws, 20260927):
        seen[ps.root_policy(t, 1, x)[0]] += 1
    for a in range(n.shape[0]):
        q = n[a] / S
        assert abs(seen[a] - draws * q) <= 5 * math.sqrt(draws * q * (1 - q)), (a, seen[a], draws * q)
    # the draw itself: k = floor((u >> 32) * S / 2^32) against the running sums, 2^31 - 1 visits included
    for S2, hi, want in ((2 ** 31 - 1, 2 ** 32 - 1, 2 ** 31 - 2), (2 ** 31 - 1, 0, 0), (3, 2 ** 31, 1)):
        assert ((hi * S2) >> 32) == want


def test_todo_protocol_and_noise_once():
    N, T, komi, c, eps = 5, 12, 0.5, 0.6, 0.25
    roots, trees = _searched(N=N, T=T, c=c, komi=komi)
    A = N * N + 1
    R = len(trees)
    z = (np.arange(R * A, dtype=np.float32).reshape(R, A) % 7 + 1) / np.float32(32)
    acts = [pa.most_visited_root(t) for t in trees]
    acts[0] = [int(a) for a in trees[0].legal[0] if trees[0].child[0, a] < 0][0]   # an unvisited action: a fresh tree
    kept = [pa.advance(t, a, pa.next_root(t, a)) for t, a in zip(trees, acts)]
    kinds = ['ended' if t.legal[0].size == 0 else ('kept' if t.n[0] > 0 else 'fresh') for t in trees]
    assert {'ended', 'kept', 'fresh'} <= set(kinds), (kinds, kept)          # the pass root: its pass child is terminal
    before = [t.prior[0].copy() for t in trees]
    todo = [ps.root_noise(t, z[r], eps, 1) for r, t in enumerate(trees)]   # before round 0: the kept roots
    for r, t in enumerate(trees):
        changed = not np.array_equal(pe.bits(t.prior[0]), pe.bits(before[r]))
        assert changed == (kinds[r] == 'kept') and todo[r] == (kinds[r] != 'kept'), (r, kinds[r])
    kept_rows = [t.prior[0].copy() for t in trees]
    pa.search_rounds(trees, 1, None, pe.hash_evaluator_np, c, komi)
    plain = [t.prior[0].copy() for t in trees]
    todo = [ps.root_noise(t, z[r], eps, todo[r]) for r, t in enumerate(trees)]   # after round 0: the fresh roots
    for r, t in enumerate(trees):
        if kinds[r] == 'kept':                                              # not a second time
            assert np.array_equal(pe.bits(t.prior[0]), pe.bits(kept_rows[r])) and todo[r] == 0
        elif kinds[r] == 'fresh':
            assert todo[r] == 0 and not np.array_equal(pe.bits(t.prior[0]), pe.bits(plain[r]))
            keep = np.float32(1) - np.float32(eps)
            for a in range(A):
                want = keep * plain[r][a] + np.float32(eps) * z[r, a] if a in t.legal[0] else np.float32(0)
                assert t.prior[0, a] == np.float32(want)
        else:                                                               # ended roots never
            assert todo[r] == 1 and np.array_equal(pe.bits(t.prior[0]), pe.bits(plain[r])) and not t.prior[0].any()
    again = [t.prior[0].copy() for t in trees]
    assert [ps.root_noise(t, z[r], eps, todo[r]) for r, t in enumerate(trees)] == todo
    assert all(np.array_equal(pe.bits(t.prior[0]), pe.bits(again[r])) for r, t in enumerate(trees))
    # the noise's odd values, and eps at its ends
    t = trees[kinds.index('kept')]
    row, legal = t.prior[0].copy(), t.legal[0]
    odd = np.resize(np.array([np.nan, -1.0, -0.0, np.inf, 0.5], np.float32), A)
    ps.root_noise(t, odd, 0.0, 1)
    for a in legal:
        assert pe.bits(t.prior[0, a:a + 1])[0] == (0x7FC00000 if np.isinf(odd[a]) else pe.bits(row[a:a + 1])[0])
    t.prior[0] = row
    ps.root_noise(t, odd, 1.0, 1)
    for a in legal:
        want = odd[a] if odd[a] > 0 else np.float32(0)
        assert pe.bits(t.prior[0, a:a + 1])[0] == pe.bits(np.array([want], np.float32))[0]


@pytest.mark.parametrize('L,sample_moves', [(None, 0), (None, 3), (4, 2)])
def test_expected_selfplay_records(L, sample_moves):
    N, T, M, komi = 5, 16, 5, 0.5
    roots = np.concatenate([mc.crafted_roots(N), mc.make_roots(N, 3, 9, max_ply=20, step=10)[1:2]])
    R, A = roots.shape[0], N * N + 1
    z = lambda mv, legal: np.where(legal, np.float32(1) / np.float32(8), np.float32(0)).astype(np.float32)
    e = ps.expected_selfplay(roots, M, T, pe.hash_evaluator_np, c=0.6, komi=komi, leaves=L, noise=z, sample_moves=sample_moves)
    sums = e['pi'].astype(np.float64).sum(axis=2)
    assert (np.abs(sums - 1) < 1e-6)[e['actions'] >= 0].all() and not e['pi'][e['actions'] < 0].any()
    assert np.array_equal(e['lengths'], (e['actions'] >= 0).sum(axis=1)) and (e['value'][e['actions'] < 0] == 0).all()
    ended = e['final_states'][:, 5, 0, 0] != 0
    assert ended.any() and (e['lengths'] < M).any() and (e['lengths'] > 0).any() and (~ended).any()
    for r in range(R):
        states = roots[r]
        for mv in range(M):                                                 # the recorded states replay the actions
            assert np.array_equal(e['states'][r, mv], states)
            a = int(e['actions'][r, mv])
            assert (a == -1) == (mv >= e['lengths'][r])
            states = pa.c_oracle.next_state(states, a) if a >= 0 else states
        assert np.array_equal(e['final_states'][r], states)
        want = int(pe.terminal_value(states, komi)) if ended[r] else 0      # the sign rule of the search's ended leaves
        assert e['outcome'][r] == want and (want != 0 or not ended[r])      # (komi 0.5: an ended game has a winner)
    draws = [(x - x0) * mc.GAMMA_INV % 2 ** 64 for x, x0 in zip(e['rng'], ps.seeds(R, 20260927))]
    assert draws == [min(int(n), sample_moves) for n in e['lengths']]       # one step per sampled move of a live root
    if sample_moves == 0:
        acts, final, _, _ = pa.expected_puct_play(roots, M, T, pe.hash_evaluator_np, c=0.6, komi=komi, leaves=L)
        plain = ps.expected_selfplay(roots, M, T, pe.hash_evaluator_np, c=0.6, komi=komi, leaves=L)
        assert np.array_equal(plain['actions'], acts) and np.array_equal(plain['final_states'], final)
