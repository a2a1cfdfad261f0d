"""CPU: UCT tree search (gg_uct_begin / _select / _backup, gogame.batch_uct) without a device - argument checks of the C-ABI,
no CPU fallback in the Python API, and the restatement the GPU tests build on (tests/mc_expect.py) checked against
the C restatement and its own invariants."""
import math

import numpy as np
import pytest

import mc_expect as mc
from oracle import c_oracle


@pytest.fixture(scope='module')
def built(native_built):
    from gymgo_amd import _lib
    return _lib


def _begin(L, R=4, N=9, I=8, K=4, ptr=1):
    p = ptr or None
    return L.gg_uct_begin(p, R, N, I, K, p, p, p, p, p, None)


def _select(L, R=4, N=9, I=8, K=4, c=1.0, ptr=1):
    p = ptr or None
    return L.gg_uct_select(R, N, I, K, c, p, p, p, p, p, p, p, p, p, None)


def _backup(L, R=4, N=9, I=8, K=4, ptr=1):
    p = ptr or None
    return L.gg_uct_backup(R, N, I, K, p, p, p, p, p, p, p, p, p, None)


def test_uct_entry_points_check_arguments_before_device_work(built):
    L = built.lib()
    for call in (_begin, _select, _backup):
        assert call(L, N=1) == -1 and call(L, N=20) == -1
        assert call(L, R=-1) == -1
        assert call(L, I=0) == -3 and call(L, I=-2) == -3
        assert call(L, K=0) == -3
        assert call(L, I=2 ** 16, K=2 ** 15) == -1                  # the root's n = I K must fit an int32
        assert call(L, I=2 ** 16 - 1, K=2 ** 15, ptr=0) == -2        # (I K = 2^31 - 2^15: allowed)
        assert call(L, ptr=0) == -2
        assert call(L, R=0, ptr=0) == -2                             # NULL buffers are an error even with nothing to do
        assert call(L, N=1, I=0, ptr=0) == -1                        # the order of gg_playouts_*: sizes, arguments, pointers
        assert call(L, I=0, ptr=0) == -3
    for c in (-1.0, -1e-300, math.inf, math.nan):
        assert _select(L, c=c) == -3
    assert _select(L, c=0.0, ptr=0) == -2
    # totals is the only optional buffer: a NULL one still leaves the other NULL buffers an error
    assert L.gg_uct_backup(4, 9, 8, 4, 1, 1, None, 1, 1, 1, 1, 1, None, None) == -2


def test_batch_uct_has_no_cpu_fallback(built):
    import torch
    from gymgo_amd import gogame
    if torch.cuda.is_available():
        pytest.skip('device present')
    for fn in (gogame.batch_uct, gogame.uct_actions):
        with pytest.raises(built.GymGoNativeError):
            fn(np.zeros((2, 6, 9, 9), np.uint8), 4, 4)
        with pytest.raises(built.GymGoNativeError):
            fn(torch.zeros((2, 6, 9, 9), dtype=torch.uint8), 4, 4)
    with pytest.raises(built.GymGoNativeError):
        gogame.uct(np.zeros((6, 9, 9), np.uint8), 4, 4)


def test_iteration_seed_is_the_generator_of_game_i(built):
    from gymgo_amd import gogame
    for seed in (0, 20260927, 2 ** 64 - 1):
        want = c_oracle.rng_seed(seed, 40)
        for i in range(40):
            assert int(mc.po_seed(seed, i)) == int(want[i]) == gogame._uct_seed(seed, i)
    assert gogame._uct_seed(7, 12345) == int(mc.po_seed(7, 12345)[()])


def test_score_is_the_float64_expression():
    L = mc.log_table(8, 16)
    assert L[0] == -np.inf and L[3] == math.log(48.0)
    u = mc.score(5, 3, 16, L[4], math.sqrt(2))
    assert u == (2.0 * 5 + 3) / (2.0 * 16) + math.sqrt(2) * math.sqrt(math.log(64) / 16)
    assert mc.score(0, 0, 4, L[1], 0.0) == 0.0


@pytest.mark.parametrize('N', [5, 9])
def test_first_iterations_expand_the_legal_actions_in_order(N):
    """With I <= |legal(root)| every iteration expands the root's next legal action, and that child's stats are exactly
    batch_playouts of the child with the iteration's seed."""
    K, seed, f0 = 3, 11, 2
    roots = np.concatenate([mc.make_roots(N, 3, 5, max_ply=N * N // 2, step=N)[1:2], mc.crafted_roots(N)[:3]])
    I = 6
    e = mc.expected_uct(roots, I, K, base_seed=seed, first_root=f0)
    mp = -(-8 * N * N // 32) * 32
    for r in range(roots.shape[0]):
        acts = mc.legal_actions(roots[r])
        assert acts.size >= I
        t = e['tree']
        assert list(t['action'][r, 1:]) == list(acts[:I]) and (t['parent'][r, 1:] == 0).all()
        assert t['parent'][r, 0] == -1 and t['action'][r, 0] == -1 and e['nodes'][r] == I + 1
        for i in range(I):
            kid = c_oracle.next_state(roots[r], int(acts[i]))
            one = mc.expected_playouts(kid[None], K, mp, base_seed=int(mc.po_seed(seed, i)), first_root=f0 + r)
            assert t['visits'][r, i + 1] == K == e['visits'][r, acts[i]]
            for k in ('black_wins', 'white_wins', 'draws'):
                assert t[k][r, i + 1] == one[k][0] == e[k][r, acts[i]], (r, i, k)
        assert e['root_visits'][r] == I * K == e['visits'][r].sum()
        for k in ('black_wins', 'white_wins', 'draws'):
            assert t[k][r, 0] == e[k][r].sum()


def test_search_invariants_and_terminal_nodes():
    """5x5, I past the root's legal actions: the root's n is I K and equal to its children's; every node's n is K plus its
    children's (K times for a terminal node: it is evaluated each time it is reached); the search reaches terminal nodes;
    shards by first_root are the whole."""
    N, K, I = 5, 2, 60
    roots = np.concatenate([mc.crafted_roots(N)[1:2], mc.make_roots(N, 3, 9, max_ply=20, step=10)[1:2]])
    e = mc.expected_uct(roots, I, K, c=0.8, base_seed=4)
    terminal_seen = 0
    for r, t in enumerate(e['trees']):
        assert e['root_visits'][r] == I * K == e['visits'][r].sum()
        n = t.stats[:, 0]
        used = len(t.boards)
        assert used == e['nodes'][r] and used <= I + 1
        for x in range(used):
            kids = t.child[x][t.child[x] >= 0]
            if t.legal[x].size:
                assert n[x] == K + n[kids].sum() or x == 0 and n[x] == n[kids].sum()
            else:
                terminal_seen += 1
                assert kids.size == 0 and n[x] % K == 0 and n[x] >= K
            assert t.stats[x, 1:].sum() == n[x]
        assert (e['tree']['visits'][r, used:] == 0).all() and (e['tree']['parent'][r, used:] == -1).all()
    assert terminal_seen > 0
    a = mc.expected_uct(roots[:1], I, K, c=0.8, base_seed=4)
    b = mc.expected_uct(roots[1:], I, K, c=0.8, base_seed=4, first_root=1)
    for k in mc.ROOT_KEYS:
        assert np.array_equal(np.concatenate([a[k], b[k]]), e[k]), k


def test_ended_root_gives_the_trivial_result():
    N, K, I = 7, 4, 5
    roots = mc.crafted_roots(N)[3:]
    e = mc.expected_uct(roots, I, K, base_seed=3)
    assert not e['legal'].any() and e['nodes'].tolist() == [1]
    assert e['root_visits'].tolist() == [I * K] and e['plies_sum'].tolist() == [0] and e['unfinished'].tolist() == [0]
    for k in ('visits', 'black_wins', 'white_wins', 'draws'):
        assert not e[k].any()
    b, w = c_oracle.batch_areas(roots)
    col = 'black_wins' if b[0] > w[0] else ('white_wins' if b[0] < w[0] else 'draws')
    assert e['tree'][col][0, 0] == I * K
    assert mc.most_visited(e).tolist() == [-1]


def test_most_visited_restatement():
    roots = mc.crafted_roots(5)
    A = 26
    res = {'legal': mc.legal_mask(roots), 'visits': np.zeros((4, A), np.int32)}
    res['visits'][:, 20] = 4                                   # (4, 0) and (4, 2): empty on the three live roots
    res['visits'][:, 22] = 4
    assert mc.most_visited(res).tolist() == [20, 20, 20, -1]
    res['visits'][2, 7] = 9                                    # (1, 2) is occupied on the ko root: not a candidate
    assert mc.most_visited(res).tolist() == [20, 20, 20, -1]
    res['visits'][:] = 0
    assert mc.most_visited(res)[:3].tolist() == [int(np.flatnonzero(res['legal'][i])[0]) for i in range(3)]
