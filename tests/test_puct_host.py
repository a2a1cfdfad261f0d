"""CPU: PUCT tree search (gg_puct_begin / _select / _backup, gogame.batch_puct / PuctSearch) without a device - argument
checks of the C-ABI, no CPU fallback in the Python API, the call order of PuctSearch, and the restatement the GPU tests
build on (tests/mc_puct_expect.py) checked against its own invariants."""
import math

import numpy as np
import pytest

import mc_expect as mc
import mc_puct_expect as pe
from oracle import c_oracle


@pytest.fixture(scope='module')
def built(native_built):
    from gymgo_amd import _lib
    return _lib


def _begin(L, R=4, N=9, I=8, ptr=1, **_):
    p = ptr or None
    return L.gg_puct_begin(p, R, N, I, p, p, p, p, p, p, None)


def _select(L, R=4, N=9, I=8, c=1.0, ptr=1, **_):
    p = ptr or None
    return L.gg_puct_select(R, N, I, c, p, p, p, p, p, p, p, p, p, None)


def _backup(L, R=4, N=9, I=8, komi=0.0, ptr=1, **_):
    p = ptr or None
    return L.gg_puct_backup(R, N, I, komi, p, p, p, p, p, p, p, p, p, None)


def test_puct_entry_points_check_arguments_before_device_work(built):
    L = built.lib()
    for call in (_begin, _select, _backup):
        assert call(L, N=1) == -1 and call(L, N=20) == -1
        assert call(L, R=-1) == -1
        assert call(L, I=0) == -3 and call(L, I=-2) == -3
        assert call(L, ptr=0) == -2
        assert call(L, R=0, ptr=0) == -2                             # NULL buffers are an error even with nothing to do
        assert call(L, N=1, I=0, ptr=0) == -1                        # the order of gg_uct_*: sizes, arguments, pointers
        assert call(L, I=0, ptr=0) == -3
        assert call(L, I=2 ** 31 - 2, ptr=0) == -2                   # (the largest I: allowed)
        assert call(L, I=2 ** 31 - 1) == -3                          # I + 1 nodes are counted in an int32
    for c in (-1.0, -1e-300, math.inf, math.nan):
        assert _select(L, c=c) == -3 and _select(L, c=c, ptr=0) == -3
    assert _select(L, c=0.0, ptr=0) == -2 and _select(L, c=1e300, ptr=0) == -2
    for komi in (math.inf, -math.inf, math.nan):
        assert _backup(L, komi=komi) == -3 and _backup(L, komi=komi, ptr=0) == -3
    assert _backup(L, komi=-7.5, ptr=0) == -2
    # every buffer is required: one NULL among them is an error
    for i in range(9):
        ptrs = [1] * 9
        ptrs[i] = None
        assert L.gg_puct_select(4, 9, 8, 1.0, *ptrs, None) == -2, i
        assert L.gg_puct_backup(4, 9, 8, 0.0, *ptrs, None) == -2, i
    for i in range(7):
        ptrs = [1] * 7
        ptrs[i] = None
        assert L.gg_puct_begin(ptrs[0], 4, 9, 8, *ptrs[1:], None) == -2, i
    assert built.lib().gg_version() == 5


def test_batch_puct_has_no_cpu_fallback(built):
    import torch
    from gymgo_amd import gogame
    if torch.cuda.is_available():
        pytest.skip('device present')
    ev = lambda states, legal: (None, None)
    for fn in (gogame.batch_puct, gogame.puct_actions):
        with pytest.raises(built.GymGoNativeError):
            fn(np.zeros((2, 6, 9, 9), np.uint8), 4, ev)
        with pytest.raises(built.GymGoNativeError):
            fn(torch.zeros((2, 6, 9, 9), dtype=torch.uint8), 4, ev)
    with pytest.raises(built.GymGoNativeError):
        gogame.puct(np.zeros((6, 9, 9), np.uint8), 4, ev)
    with pytest.raises(built.GymGoNativeError):
        gogame.PuctSearch(np.zeros((2, 6, 9, 9), np.uint8), 4)
    with pytest.raises(ValueError):
        gogame.playout_evaluator(0, komi=0.0)
    with pytest.raises(ValueError):
        gogame.playout_evaluator(4, policy='eyes', komi=0.0)
    with pytest.raises(ValueError):
        gogame.playout_evaluator(4, komi=math.nan)
    with pytest.raises(TypeError):
        gogame.playout_evaluator(4)                                   # komi has no default: it must be the search's
    ev = gogame.playout_evaluator(4, policy='no_eye_fill', komi=7.5)
    assert callable(ev) and ev.komi == 7.5
    with pytest.raises(ValueError):                                   # ... and batch_puct holds it to that, before any device work
        gogame.batch_puct(np.zeros((2, 6, 9, 9), np.uint8), 4, ev, komi=0.0)


def test_puct_search_call_order(built, monkeypatch):
    """select / backup alternate, at most `iterations` times; result() only with no leaf outstanding.  The order is host
    state: checked here on a search object whose device work is stubbed out (R = 0 needs no launch)."""
    import torch
    from gymgo_amd import gogame
    monkeypatch.setattr(gogame, '_device', lambda: torch.device('cpu'))
    s = gogame.PuctSearch(np.zeros((0, 6, 5, 5), np.uint8), 2, c=0.5, komi=0.5)
    A = 26
    p, v = np.zeros((0, A), np.float32), np.zeros(0, np.float32)
    with pytest.raises(ValueError):
        s.backup(p, v)                       # nothing handed out yet
    assert s.result().visits.shape == (0, A)  # nothing outstanding: allowed
    states, legal = s.select()
    assert tuple(states.shape) == (0, 6, 5, 5) and tuple(legal.shape) == (0, A) and legal.dtype == torch.bool
    with pytest.raises(ValueError):
        s.select()                           # twice in a row
    with pytest.raises(ValueError):
        s.result()                           # a leaf is outstanding
    with pytest.raises(ValueError):
        s.backup(np.zeros((1, A), np.float32), v)   # wrong shape: still outstanding afterwards
    s.backup(p, v)
    with pytest.raises(ValueError):
        s.backup(p, v)
    s.select()
    s.backup(p, v)
    assert s.iterations_done == 2
    with pytest.raises(ValueError):
        s.select()                           # all iterations done
    res = s.result(tree=True)
    assert isinstance(res.visits, np.ndarray) and res.tree.parent.shape == (0, 3) and res.value_sum.dtype == np.float64
    for bad in (dict(iterations=0), dict(c=-1.0), dict(c=math.inf), dict(c=math.nan), dict(komi=math.nan), dict(komi=math.inf),
                dict(iterations=2 ** 31), dict(iterations=2 ** 31 - 1)):
        kw = dict(iterations=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            gogame.PuctSearch(np.zeros((0, 6, 5, 5), np.uint8), **kw)
    with pytest.raises(ValueError):
        gogame.PuctSearch(np.zeros((0, 5, 5, 5), np.uint8), 2)


def test_score_is_the_float64_expression():
    u = pe.score(-1.0, 3.25, 4, np.float32(0.3), 9, 1.25)
    assert u == (-1.0 * 3.25 / 4.0) + ((1.25 * float(np.float32(0.3))) * math.sqrt(9.0)) / 5.0
    assert pe.score(1.0, 0.0, 0, np.float32(0.5), 1, 2.0) == 1.0          # a fresh node: sqrt(1), the prior decides
    assert pe.score(1.0, 7.0, 0, np.float32(0.0), 5, 2.0) == 0.0          # no visits: q = 0 whatever w holds
    assert pe.score(1.0, 0.0, 0, np.float32(np.inf), 4, 1.0) == math.inf
    assert pe.score(1.0, 0.0, 0, np.float32(np.inf), 4, 0.0) == -math.inf  # 0 * inf = NaN counts as -inf


def test_evaluators_are_integer_hashes():
    roots = mc.make_roots(7, 6, 21, max_ply=40, step=8)
    legal = mc.legal_mask(roots)
    p, v = pe.hash_evaluator_np(roots, legal)
    assert p.dtype == np.float32 and v.dtype == np.float32 and p.shape == legal.shape and v.shape == (6,)
    assert not p[~legal].any() and ((p * 256) % 1 == 0).all() and (p >= 0).all() and (p < 1).all()
    assert ((v * 128) % 1 == 0).all() and (np.abs(v) <= 1).all() and len(set(v.tolist())) > 1
    p2, v2 = pe.hash_evaluator_np(roots[::-1], legal[::-1])
    assert np.array_equal(p2[::-1], p) and np.array_equal(v2[::-1], v)   # row-wise: no dependence on the batch
    hp, hv = pe.hostile_evaluator_np(mc.make_roots(9, 40, 5, max_ply=60, step=3), np.ones((40, 82), bool))
    assert np.isnan(hp).any() and (hp < 0).any() and np.isposinf(hp).any() and np.isneginf(hp).any()
    assert (hp == 0).all(axis=1).any() and (np.abs(hv[np.isfinite(hv)]) > 1).any()
    assert np.isnan(hv).any() or np.isinf(hv).any()


@pytest.mark.parametrize('evaluator', [pe.hash_evaluator_np, pe.hostile_evaluator_np])
def test_search_invariants(evaluator):
    """5x5, I far past the root's actions: root n = I, the children's n sum to I - 1 at a live root, priors zero on illegal
    actions, child ids above their parent's, every node's n = its own evaluations + its children's n, every node's w = the
    sum of the evaluations in its subtree (exact: the values are multiples of 1 / 128, or +-1 at ended nodes), ended
    nodes inside the tree are revisited; shards by root are the whole."""
    N, I = 5, 150
    roots = np.concatenate([mc.crafted_roots(N)[:3], mc.make_roots(N, 3, 9, max_ply=20, step=10)[1:2]])
    e = pe.expected_puct(roots, I, evaluator, c=0.6, komi=0.5)
    ended_revisited = 0
    for r, t in enumerate(e['trees']):
        used = len(t.boards)
        assert e['root_visits'][r] == I and e['visits'][r].sum() == I - 1 and used == e['nodes'][r] <= I + 1
        assert not e['priors'][r][~e['legal'][r]].any() and not e['visits'][r][~e['legal'][r]].any()
        assert np.isfinite(t.w).all()
        total = [sum(t.evals[x]) for x in range(I + 1)]
        for x in range(used - 1, -1, -1):          # children have larger ids: their subtree sums are complete first
            kids = t.child[x][t.child[x] >= 0]
            assert (kids > x).all() and (t.parent[kids] == x).all()
            ok = np.zeros(N * N + 1, bool)
            ok[t.legal[x]] = True
            assert not t.prior[x][~ok].any() and (t.prior[x] >= 0).all() and not np.isnan(t.prior[x]).any()
            assert t.n[x] == len(t.evals[x]) + t.n[kids].sum()
            if t.legal[x].size:
                assert len(t.evals[x]) == 1 and abs(t.evals[x][0]) <= 1
            else:
                assert kids.size == 0 and set(t.evals[x]) <= {-1.0, 0.0, 1.0} and len(set(t.evals[x])) == 1
                ended_revisited += len(t.evals[x]) > 1
            if x:
                total[t.parent[x]] += total[x]
            assert t.w[x] == total[x], (r, x)
        assert (t.n[used:] == 0).all() and (t.parent[used:] == -1).all() and not t.prior[used:].any()
    assert ended_revisited > 0
    a = pe.expected_puct(roots[:1], I, evaluator, c=0.6, komi=0.5)
    b = pe.expected_puct(roots[1:], I, evaluator, c=0.6, komi=0.5)
    for k in pe.ROOT_KEYS:
        assert np.array_equal(pe.bits(np.concatenate([a[k], b[k]])), pe.bits(e[k])), k


def test_ended_root_creates_no_nodes():
    N, I = 7, 5
    roots = mc.crafted_roots(N)[3:]
    for komi in (0.0, 0.5, -0.5):
        e = pe.expected_puct(roots, I, pe.hash_evaluator_np, komi=komi)
        assert not e['legal'].any() and e['nodes'].tolist() == [1] and e['root_visits'].tolist() == [I]
        assert not e['visits'].any() and not e['priors'].any() and not e['value_sum'].any()
        b, w = c_oracle.batch_areas(roots)
        x = float(b[0]) - float(w[0]) - komi
        assert e['root_value_sum'].tolist() == [I * float(np.sign(x))]
        assert pe.most_visited(e).tolist() == [-1]


def test_a_certain_prior_is_followed_every_iteration():
    """One legal action with prior 1, the rest 0, values 0: q = 0 everywhere, so U > 0 on that action alone - every
    iteration descends the same line and adds one node to its end."""
    N, I = 5, 12
    root = mc.crafted_roots(N)[:1]

    def evaluator(states, legal):
        p = np.zeros(legal.shape, np.float32)
        for i in range(legal.shape[0]):
            p[i, np.flatnonzero(legal[i])[3]] = 1     # (not the lowest action: the tie-break would pick that one anyway)
        return p, np.zeros(legal.shape[0], np.float32)

    e = pe.expected_puct(root, I, evaluator, c=1.25)
    t = e['trees'][0]
    assert e['nodes'][0] == I and list(t.parent[:I]) == [-1] + list(range(I - 1))
    assert list(t.n[:I]) == list(range(I, 0, -1)) and not t.w.any()
    for x in range(1, I):
        assert t.action[x] == np.flatnonzero(mc.legal_mask(t.boards[x - 1][None])[0])[3]
    assert e['visits'][0].sum() == I - 1 == e['visits'][0, t.action[1]]
