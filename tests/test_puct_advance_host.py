"""CPU: tree reuse across moves (gg_puct_advance, gogame.PuctSearch(.., capacity=) / advance / root_states, puct_play) without
a device - the argument checks of the C-ABI in their stated order, the ValueError cases of `capacity` and `advance`, the call
order at R = 0, and the restatement the GPU tests build on (tests/mc_puct_advance_expect.py): after an advance the kept
count is the size of the child's subtree, n_x = 1 + the children's n at every kept live node, child ids exceed their
parent's, the kept root's board is the C restatement's next_state, -1 changes nothing, an unvisited legal action and an ended
root give the fresh tree.  The inputs are asserted to contain a kept subtree of more than one level, a kept count of exactly
1, a fresh tree from a legal unvisited action and, on 5x5, a kept subtree with ended nodes in it."""
import copy

import numpy as np
import pytest

import mc_expect as mc
import mc_puct_expect as pe
import mc_puct_advance_expect as pa
from oracle import c_oracle


@pytest.fixture(scope='module')
def built(native_built):
    from gymgo_amd import _lib
    return _lib


def _advance(L, R=4, N=9, C=8, ptrs=None, kept=1):
    p = [1] * 10 if ptrs is None else ptrs
    return L.gg_puct_advance(p[0], p[1], R, N, C, p[2], p[3], p[4], p[5], p[6], p[7], p[8], kept or None, None)


def test_advance_entry_point_checks_arguments_before_device_work(built):
    L = built.lib()
    none = [None] * 10
    assert _advance(L, N=1) == -1 and _advance(L, N=20) == -1 and _advance(L, R=-1) == -1
    assert _advance(L, C=0) == -3 and _advance(L, C=-2) == -3 and _advance(L, C=2 ** 31 - 1) == -3
    assert _advance(L, ptrs=none) == -2 and _advance(L, R=0, ptrs=none) == -2   # NULL buffers are an error even with nothing to do
    assert _advance(L, N=1, C=0, ptrs=none) == -1                              # sizes, arguments, pointers
    assert _advance(L, C=0, ptrs=none) == -3
    assert _advance(L, C=2 ** 31 - 2, ptrs=none) == -2                         # (the largest capacity: allowed)
    for i in range(9):                                                         # every buffer but kept is required
        ptrs = [1] * 10
        ptrs[i] = None
        assert _advance(L, ptrs=ptrs) == -2, i
        assert _advance(L, R=0, ptrs=ptrs) == -2, i
    assert _advance(L, R=0) == 0 and _advance(L, R=0, kept=0) == 0             # R = 0 is no work; kept may be NULL
    assert 'gg_puct_advance' in built.EXPORTS
    assert L.gg_version() == 5


def test_capacity_and_advance_errors_and_call_order_without_a_device(built, monkeypatch):
    import torch
    from gymgo_amd import gogame
    monkeypatch.setattr(gogame, '_device', lambda: torch.device('cpu'))
    empty = np.zeros((0, 6, 5, 5), np.uint8)
    A = 26
    p, v = np.zeros((0, A), np.float32), np.zeros(0, np.float32)
    for leaves, least in ((None, 5), (1, 5), (3, 13)):
        for bad in (least - 1, 0, -1, 2 ** 31, 7.0, '9', True):
            with pytest.raises(ValueError):
                gogame.PuctSearch(empty, 4, leaves=leaves, capacity=bad)
            with pytest.raises(ValueError):
                gogame.batch_puct(empty, 4, lambda s, l: (p, v), leaves=leaves, capacity=bad)
            with pytest.raises(ValueError):
                gogame.puct_play(empty, 1, 4, lambda s, l: (p, v), leaves=leaves, capacity=bad)
        assert gogame.PuctSearch(empty, 4, leaves=leaves)._C == least - 1                       # None: today's size
        assert gogame.PuctSearch(empty, 4, leaves=leaves, capacity=least)._C == least - 1
        assert gogame.PuctSearch(empty, 4, leaves=leaves, capacity=np.int64(40))._C == 39
        assert gogame.PuctSearch(empty, 4, leaves=leaves, capacity=2 ** 31 - 1)._C == 2 ** 31 - 2   # (R = 0: no memory)
        got = gogame.batch_puct(empty, 4, lambda s, l: (p, v), leaves=leaves, capacity=40, tree=True)
        assert got.tree.parent.shape == (0, 40) and got.tree.value_sum.dtype == np.float64
    s = gogame.PuctSearch(empty, 2, capacity=9)
    none = np.zeros(0, np.int64)
    kept = s.advance(none)                                    # before the first round: allowed, nothing is outstanding
    assert isinstance(kept, torch.Tensor) and kept.dtype == torch.int32 and tuple(kept.shape) == (0,)
    assert s.root_states().shape == (0, 6, 5, 5) and isinstance(s.root_states(), np.ndarray)
    for bad in (np.zeros(1, np.int64), np.zeros((0, 1), np.int64), np.zeros(0, np.float32), np.zeros(0, bool)):
        with pytest.raises(ValueError):
            s.advance(bad)
    s.select()
    with pytest.raises(ValueError):
        s.advance(none)                                       # a select is outstanding
    with pytest.raises(ValueError):
        s.root_states()
    s.backup(p, v)
    s.select()
    s.backup(p, v)
    with pytest.raises(ValueError):
        s.select()                                            # all rounds done
    s.advance(torch.zeros(0, dtype=torch.int32))
    assert s.iterations_done == 0
    s.select()                                                # ... and `iterations` more may follow
    s.backup(p, v)
    s.advance(none, iterations=1, check=False)
    s.select()
    s.backup(p, v)
    with pytest.raises(ValueError):
        s.select()
    for bad in (0, -3, 2 ** 31):
        with pytest.raises(ValueError):
            s.advance(none, iterations=bad)
    s.advance(none)                                           # the default is the constructor's 2, not the last advance's 1
    for _ in range(2):
        s.select()
        s.backup(p, v)
    with pytest.raises(ValueError):
        s.select()
    calls = []

    def ev(states, legal):
        calls.append((tuple(states.shape), tuple(legal.shape)))
        return p, v

    for reuse in (True, False):
        del calls[:]
        acts, final = gogame.puct_play(empty, 3, 2, ev, leaves=2, capacity=30, reuse=reuse)
        assert calls == [((0, 6, 5, 5), (0, A))] * 6
        assert isinstance(acts, np.ndarray) and acts.shape == (0, 3) and acts.dtype == np.int64
        assert isinstance(final, np.ndarray) and final.shape == (0, 6, 5, 5) and final.dtype == np.uint8
    with pytest.raises(ValueError):
        gogame.puct_play(empty, -1, 2, ev)
    ev.komi = 7.5
    with pytest.raises(ValueError):
        gogame.puct_play(empty, 1, 2, ev, komi=0.5)           # batch_puct's guard


def _check_kept_tree(t, N):
    """The invariants of a tree outside a round, kept or not."""
    used = len(t.boards)
    assert t.parent[0] == -1 and t.action[0] == -1
    for x in range(used):
        kids = t.child[x][t.child[x] >= 0]
        assert (kids > x).all() and (kids < used).all() and (t.parent[kids] == x).all()
        assert (t.action[kids] == np.flatnonzero(t.child[x] >= 0)).all()
        if t.legal[x].size and t.n[x] > 0:
            assert t.n[x] == 1 + t.n[kids].sum(), x              # a live node is evaluated once: n_x = 1 + the children's n
        assert t.n[x] == len(t.evals[x]) + t.n[kids].sum(), x
        for a in np.flatnonzero(t.child[x] >= 0):
            assert np.array_equal(t.boards[t.child[x, a]], c_oracle.next_state(t.boards[x], int(a)))
        ok = np.zeros(N * N + 1, bool)
        ok[t.legal[x]] = True
        assert not t.prior[x][~ok].any()
    assert (t.n[used:] == 0).all() and (t.w[used:] == 0).all() and (t.parent[used:] == -1).all() and (t.action[used:] == -1).all()
    assert (t.child[used:] == -1).all() and not t.prior[used:].any()


def _snapshot(t):
    return [np.array(getattr(t, k)).copy() for k in ('parent', 'action', 'n', 'w', 'prior', 'child')] + [np.stack(t.boards)]


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(pe.bits(x), pe.bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize('L', [None, 1, 4])
def test_advance_on_the_restatement(L):
    N, T, c, komi = 5, 60, 0.6, 0.5
    A = N * N + 1
    roots = np.concatenate([mc.crafted_roots(N)[:3], mc.make_roots(N, 3, 9, max_ply=20, step=10)[1:2], mc.crafted_roots(N)[3:]])
    R = roots.shape[0]
    ended_root = [r for r in range(R) if mc.legal_actions(roots[r]).size == 0]
    assert ended_root
    seen = dict(deep=0, one=0, fresh=0, ended_inside=0, stay=0, ended_root=0)
    for pick in ('most', 'least', 'unvisited', 'stay'):
        trees = pa.make_trees(roots, 2 * T * (L or 1) + 1, L)
        pa.search_rounds(trees, T, L, pe.hash_evaluator_np, c, komi)
        for r, t in enumerate(trees):
            _check_kept_tree(t, N)
            before, m = _snapshot(t), len(t.boards)
            acts = t.legal[0]
            kids = [int(a) for a in acts if t.child[0, a] >= 0]
            if r in ended_root:
                # an ended root has no children: -1 keeps it, anything else starts afresh on the board the caller supplies
                assert pa.advance(t, -1, None) == m == 1 and _same(before, _snapshot(t))
                assert pa.advance(t, A - 1, t.boards[0]) == 0 and len(t.boards) == 1 and t.n[0] == 0 and not t.prior[0].any()
                seen['ended_root'] += 1
                continue
            if pick == 'stay':
                assert pa.advance(t, -1, None) == m and _same(before, _snapshot(t)) and not hasattr(t, 'zeroed')
                seen['stay'] += 1
                continue
            if pick == 'unvisited':
                free = [int(a) for a in acts if t.child[0, a] < 0]
                if not free:
                    continue
                a = free[0]
                nxt = c_oracle.next_state(t.boards[0], a)
                assert pa.advance(t, a, nxt) == 0
                fresh = (pe.Tree if L is None else pa.pl.LeavesTree)(nxt, t.I)
                assert _same(_snapshot(t), _snapshot(fresh)) and len(t.boards) == 1 and t.zeroed == m
                seen['fresh'] += 1
                continue
            by_n = sorted(kids, key=lambda a: (int(t.n[t.child[0, a]]), a))
            a = by_n[-1] if pick == 'most' else by_n[0]
            k = int(t.child[0, a])
            sub = pa.subtree(t, k)
            old = copy.deepcopy(t)
            kept = pa.advance(t, a, None)
            assert kept == len(sub) == len(t.boards) and t.zeroed == m
            _check_kept_tree(t, N)
            assert np.array_equal(t.boards[0], c_oracle.next_state(old.boards[0], a))
            for j, x in enumerate(sub):                          # order-preserving: node j is the j-th node of the subtree
                assert np.array_equal(t.boards[j], old.boards[x]) and t.n[j] == old.n[x]
                assert np.float64(t.w[j]).view(np.int64) == np.float64(old.w[x]).view(np.int64)
                assert np.array_equal(pe.bits(t.prior[j]), pe.bits(old.prior[x])) and t.action[j] == (old.action[x] if j else -1)
                assert np.array_equal(t.child[j] >= 0, old.child[x] >= 0)
            assert t.n[0] == old.n[k] and (t.n[m:] == old.n[m:]).all()
            depth = max(len(_chain(t, j)) for j in range(kept))
            seen['deep'] += depth > 2
            seen['one'] += kept == 1
            seen['ended_inside'] += any(t.legal[j].size == 0 for j in range(kept))
            # the search goes on from the kept tree: the new root is evaluated, so the next select scores at once
            pa.search_rounds([t], 5, L, pe.hash_evaluator_np, c, komi)
            _check_kept_tree(t, N)
            assert t.n[0] > old.n[k]
    assert all(seen.values()), seen


def _chain(t, x):
    out = [x]
    while t.parent[out[-1]] >= 0:
        out.append(int(t.parent[out[-1]]))
    return out


def test_expected_puct_play_reuse_and_fresh():
    """The move loop: with reuse the root visits before move i + 1 start at the kept child's n; without it every move starts
    at 0 and equals a loop over expected_puct on the states played so far.  A tree of the default capacity is full after the
    first move: it expands nothing more (the no-room rule) and keeps refining values."""
    N, T, M = 5, 30, 4
    roots = np.concatenate([mc.crafted_roots(N)[:2], mc.crafted_roots(N)[3:]])
    kepts, starts = [], []

    def on_move(mv, ts, a, k):
        kepts.append(list(k))
        starts.append([int(t.n[0]) for t in ts])

    acts, final, per_move, trees = pa.expected_puct_play(roots, M, T, pe.hash_evaluator_np, c=0.6, komi=0.5, capacity=4 * T,
                                                         on_move=on_move)
    assert acts.shape == (roots.shape[0], M) and (acts[-1] == -1).all() and np.array_equal(final[-1], roots[-1])
    for mv in range(1, M):                                    # every round adds one visit to a root: T on top of what was kept
        assert (per_move[mv]['root_visits'] == np.array(starts[mv - 1]) + T).all()
    assert max(max(k[:2]) for k in kepts) > 1 and max(max(s[:2]) for s in starts) > 1
    states = roots.copy()
    want = np.zeros_like(acts)
    for mv in range(M):
        e = pe.expected_puct(states, T, pe.hash_evaluator_np, c=0.6, komi=0.5)
        want[:, mv] = pe.most_visited(e)
        states = np.stack([s if a < 0 else c_oracle.next_state(s, int(a)) for s, a in zip(states, want[:, mv])])
    a2, f2, _, _ = pa.expected_puct_play(roots, M, T, pe.hash_evaluator_np, c=0.6, komi=0.5, reuse=False)
    assert np.array_equal(a2, want) and np.array_equal(f2, states)
    full = []
    pa.expected_puct_play(roots[:2], 3, T, pe.hash_evaluator_np, c=0.6, komi=0.5,
                          on_move=lambda mv, ts, a, k: full.append([len(t.boards) for t in ts]))
    _, _, per, ts = pa.expected_puct_play(roots[:2], 3, T, pe.hash_evaluator_np, c=0.6, komi=0.5)
    assert (per[1]['nodes'] == T + 1).all() and (per[2]['nodes'] == T + 1).all()        # full, and searched on
    assert (per[2]['root_visits'] >= T).all()
