"""-m gpu: the Gumbel root rule of the PUCT search (gogame.PuctSearch(gumbel=) / gumbel_root / puct_play(gumbel=) /
puct_selfplay(gumbel=): gg_gumbel_begin / gg_gumbel_select_leaves / gg_gumbel_root) against the restatement
(tests/mc_gumbel_expect.py), in lockstep: after every select() the leaf ids, moves and the live mask, after every backup() the
whole tree - links, n, w as bit patterns, v, child tables, priors as bit patterns, nodes - and done and seen; the read-out's
actions, q, visits and value exactly, and the improved policy within 1 float32 ulp of NumPy's float64 softmax of the same
read-back inputs (both sides are float64 softmaxes of at most 362 terms, and the cast may fall either side of one rounding
boundary).  base = g + log(prior) is torch's and not bit-defined: the restatement is handed the tensor the device made.

Every board size 2 .. 19 with one and three slots; N in {5, 9, 19} with L in {1, 3, 8} and m in {1, 2, 4, 16, A + 5};
c_scale in {0, 0.5} and c_visit in {0, 50}; hand-made base rows (-inf, +inf, NaN, all equal); ended roots and roots with one
legal action; three moves with advance in between, with and without set_gumbel, past the schedule and past capacity; the
plane families, symmetry and the history switched on; the move loops; the defaults; 533 roots in a child process sized for one
compute unit (later trips of the grid-stride loop)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mc_cases as cs
import mc_expect as mc
import mc_gumbel_expect as ge
import mc_puct_expect as pe
import mc_puct_leaves_expect as pl


def _device_state(s):
    """What ge.Search.state() holds, read from a gogame.PuctSearch."""
    import torch
    return {'parent': s._links[..., 0], 'action': s._links[..., 1], 'n': s._stats[..., 2], 'w': s._stats.view(torch.float64)[..., 0],
            'v': s._stats[..., 3], 'child': s._child, 'prior': s._prior, 'nodes': s._nodes, 'done': s._sims, 'seen': s._seen}


def _same(got, want, tag):
    for k, w in want.items():
        g = mc.to_np(got[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, k, g.shape, g.dtype, w.shape, w.dtype)
        assert np.array_equal(pe.bits(g), pe.bits(w)), (tag, k, np.argwhere(pe.bits(g) != pe.bits(w))[:8])


class Pair:
    """A gogame.PuctSearch(gumbel=) and its restatement, driven together."""

    def __init__(self, roots, T, L, m, name, n=None, c=1.25, komi=0.5, c_visit=50.0, c_scale=0.5, capacity=None, **search_kw):
        from gymgo_amd import gogame
        self.ev_np, self.ev_t = ge.EVALUATORS[name]
        self.bases = []
        self.dev = gogame.PuctSearch(mc.to_dev(roots), T, c=c, komi=komi, leaves=L, capacity=capacity,
                                     gumbel=gogame.Gumbel(m, n, c_visit, c_scale), **search_kw)
        self.exp = ge.Search(roots, T, L, m, n=n, c=c, komi=komi, c_visit=c_visit, c_scale=c_scale, capacity=capacity,
                             base_of=lambda s: self.bases.pop(0))
        self.R, self.L = roots.shape[0], L or 1
        self.check('begin')

    def check(self, tag):
        _same(_device_state(self.dev), self.exp.state(), tag)

    def set_g(self, g):
        self.dev.set_gumbel(g)
        self.exp.set_g(g)

    def hand(self, rows):
        """Hand-made base rows (float32 [R, A]) on both sides, once select() has stopped refreshing the tensor."""
        import torch
        assert self.dev._since >= 2 and self.exp.since >= 2
        self.dev.base.copy_(torch.from_numpy(rows).to(self.dev.base.device))
        for r, t in enumerate(self.exp.trees):
            t.base = rows[r].copy()

    def round(self, tag):
        refresh = self.dev._since < 2
        handed = self.dev.select()
        if refresh:
            self.bases.append(mc.to_np(self.dev.base).copy())
        self.exp.round(self.ev_np)
        assert not self.bases
        ids, moves = self.exp.rounds[-1]
        assert np.array_equal(mc.to_np(self.dev._leaf_id).reshape(self.R, self.L), ids), (tag, 'leaf_id')
        assert np.array_equal(mc.to_np(self.dev._move).reshape(self.R, self.L), moves), (tag, 'move')
        assert np.array_equal(mc.to_np(self.dev.live), ids >= 0), (tag, 'live')
        self.dev.backup(*self.ev_t(*handed))
        self.check(tag)

    def rounds(self, k, tag):
        for i in range(k):
            self.round((tag, i))

    def readout(self, tag):
        """-> the actions (NumPy int32 [R]) after comparing everything the read-out gives."""
        acts, q, vis, val, pi = self.exp.readout()
        s = self.dev
        g_acts, g_pi, g_val = s.gumbel_root()
        assert not self.bases
        import torch
        assert g_acts.dtype == torch.int32 and g_pi.dtype == torch.float32 and g_val.dtype == torch.float32
        assert np.array_equal(mc.to_np(g_acts), acts), (tag, mc.to_np(g_acts), acts)
        assert np.array_equal(pe.bits(g_val), pe.bits(val)), tag
        # q and visits: the entry point's own rows
        R, A, dev = self.R, q.shape[1], s._dev
        dq, dn = torch.empty((R, A), dtype=torch.float32, device=dev), torch.empty((R, A), dtype=torch.int32, device=dev)
        da, dv = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.float32, device=dev)
        from gymgo_amd import _lib
        boards, child, _, _, stats, nodes = s._tree
        if R:
            _lib.call('gg_gumbel_root', R, s._N, s._C, boards, child, stats, nodes, s.base, s._seen, s._gumbel.c_visit,
                      s._gumbel.c_scale, da, dq, dn, dv, _lib.current_raw_stream(dev))
            assert np.array_equal(pe.bits(dq), pe.bits(q)) and np.array_equal(mc.to_np(dn), vis), tag
            assert np.array_equal(mc.to_np(da), acts) and np.array_equal(pe.bits(dv), pe.bits(val)), tag
        # the improved policy: NumPy's float64 softmax of the read-back inputs, within 1 ulp; exact zeros off the legal set
        legal = mc.to_np(s._legal_roots)
        prior = mc.to_np(s._prior[:, 0, :])
        got = mc.to_np(g_pi)
        for r in range(R):
            want = ge.improved_policy(prior[r], mc.to_np(dq)[r], mc.to_np(dn)[r], legal[r], s._gumbel.c_visit, s._gumbel.c_scale)
            assert ge.ulps(got[r], want).max() <= 1, (tag, r, ge.ulps(got[r], want).max())
            assert not pe.bits(got[r][~legal[r]]).any(), (tag, r)
            if legal[r].any():
                assert abs(float(got[r].astype(np.float64).sum()) - 1.0) < 1e-5, (tag, r)
            assert np.array_equal(want, pi[r]), (tag, r)     # (the restatement's own rows are the device's, bit for bit)
        assert s.gumbel_root(pi=False)[1] is None
        return acts

    def advance(self, acts, tag):
        import torch
        kept = self.dev.advance(torch.from_numpy(np.asarray(acts, np.int64)))
        want = self.exp.advance(acts)
        assert mc.to_np(kept).tolist() == want, (tag, mc.to_np(kept).tolist(), want)
        self.check((tag, 'advance'))
        return want


pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- sizes and slots
@pytest.mark.parametrize('L', [1, 3])
@pytest.mark.parametrize('N', cs.SIZES)
def test_every_board_size(N, L):
    roots, name = ge.size_case(N, L)
    p = Pair(roots, ge.SIZE_ROUNDS, L, ge.SIZE_M, name)
    p.rounds(ge.SIZE_ROUNDS, (N, L))
    acts = p.readout((N, L))
    assert acts[-1] == -1 and (acts[:-1] >= 0).all()                 # the ended root, and the live ones
    done = mc.to_np(p.dev._sims)
    assert done[-1] == 0 and (done[:-1] <= (ge.SIZE_ROUNDS - 1) * L).all() and (done[:-1] >= 1).all()


@pytest.mark.parametrize('L', ge.SLOT_LEAVES)
@pytest.mark.parametrize('N', ge.SLOT_SIZES)
def test_slots_and_considered_actions(N, L):
    for m in ge.slot_considered(N):
        roots, name = ge.slot_case(N, L, m)
        p = Pair(roots, ge.SLOT_ROUNDS, L, m, name)
        p.rounds(ge.SLOT_ROUNDS, (N, L, m))
        p.readout((N, L, m))
        if L == 1:                                                   # one slot never collides: the whole budget is handed out
            assert mc.to_np(p.dev._sims)[:2].tolist() == [ge.SLOT_ROUNDS - 1] * 2


# ---------------------------------------------------------------- parameters and hand-made inputs
@pytest.mark.parametrize('c_visit', [0.0, 50.0])
@pytest.mark.parametrize('c_scale', [0.0, 0.5])
def test_c_visit_and_c_scale(c_visit, c_scale):
    N, T, L = 9, 8, 3
    roots = cs.stack(N, ('mid0', 'mid1', 'late0', 'ko', 'ended'))
    p = Pair(roots, T, L, 4, 'hash', c_visit=c_visit, c_scale=c_scale)
    p.set_g(ge.dyadic_g(5, N * N + 1, salt=int(c_visit + 7 * c_scale)))
    p.rounds(T, (c_visit, c_scale))
    p.readout((c_visit, c_scale))


def test_hand_made_base_rows():
    """-inf, +inf and NaN entries and rows of all-equal values (ties to the lowest action; a row of -inf throughout)."""
    N, T, L = 5, 10, 3
    A = N * N + 1
    roots = np.repeat(cs.stack(N, ('empty',)), 6, axis=0)
    p = Pair(roots, T, L, 4, 'hash', c_scale=0.5)
    p.rounds(2, 'before')
    rows = ge.dyadic_g(6, A, salt=3)
    rows[0, ::3] = -np.inf
    rows[1, 5:9] = np.inf
    rows[2, 1::2] = np.nan
    rows[3, :] = np.float32(0.25)
    rows[4, :] = -np.inf
    rows[5, :] = np.nan
    p.hand(rows)
    p.rounds(T - 2, 'hand-made')
    assert p.exp.events()['tie'] > 0 and p.exp.events()['neg_inf'] > 0
    acts = p.readout('hand-made')
    assert (acts >= 0).all()


def test_ended_roots_and_roots_with_one_legal_action():
    N, T, L = 5, 6, 3
    roots = cs.stack(N, ('ended', 'played_out', 'forced_black', 'forced_white', 'ended'))
    legal = [mc.legal_actions(r).size for r in roots]
    assert legal == [0, 0, 3, 1, 0]                                   # two eyes and the pass for black; for white the pass alone
    p = Pair(roots, T, L, 4, 'hash')
    p.rounds(T, 'ended')
    acts = p.readout('ended')
    assert acts[[0, 1, 3, 4]].tolist() == [-1, -1, N * N, -1] and acts[2] >= 0
    assert mc.to_np(p.dev._sims)[[0, 1, 4]].tolist() == [0, 0, 0] and p.exp.events()['fallback'] > 0


# ---------------------------------------------------------------- across moves
@pytest.mark.parametrize('with_g', [False, True])
@pytest.mark.parametrize('N', [5, 19])
def test_three_moves_with_advance(N, with_g):
    """Kept roots (non-zero seen), fresh trees, a root that stays (-1) and an ended one; the second and third move run past
    the schedule of a fresh root; set_gumbel only where it is allowed."""
    import torch
    T, L = 4, 3
    A = N * N + 1
    roots = cs.stack(N, ('mid0', 'late0', 'empty', 'ended'))
    p = Pair(roots, T, L, 4, 'hash', capacity=3 * T * L + 1)
    seen_kept = past = 0
    for mv in range(3):
        if with_g:
            p.set_g(ge.dyadic_g(4, A, mv))
        p.rounds(T, (N, mv))
        with pytest.raises(ValueError):
            p.dev.set_gumbel(torch.zeros((4, A)))                    # not after a select()
        acts = p.readout((N, mv))
        if mv == 1:
            acts[2] = -1                                             # this root does not move
        kept = p.advance(acts, (N, mv))
        seen_kept += int(mc.to_np(p.dev._seen).any())
        past = p.exp.events()['past']
        assert kept[3] == 1 and not mc.to_np(p.dev._sims).any()
    assert seen_kept > 0 and past > 0
    with pytest.raises(ValueError):
        p.dev.add_root_noise(torch.zeros((4, A), device='cuda'))


def test_past_the_schedule_and_past_capacity():
    """A schedule of three simulations under nine rounds of two slots; then the same roots stay (advance with -1) until the
    trees are full: the no-room rule below the root rule, nodes stay at capacity."""
    N, T, L = 5, 9, 2
    roots = cs.stack(N, ('mid0', 'late1', 'empty'))
    p = Pair(roots, T, L, 4, 'hostile', n=3)
    p.rounds(T, 'past the schedule')
    assert p.exp.events()['past'] > 0
    p.readout('past the schedule')
    full = 0
    for k in range(2):
        p.advance([-1, -1, -1], ('stay', k))
        p.rounds(T, ('stay', k))
        full = int((mc.to_np(p.dev._nodes) == T * L + 1).sum())
    assert full > 0 and (mc.to_np(p.dev._nodes) <= T * L + 1).all()
    p.readout('full')


# ---------------------------------------------------------------- host loops
def test_planes_symmetry_and_history_leave_the_tree_alone():
    """features=, symmetry= and past= on: the tree equals the tree of the same search without them, the evaluator being the
    hash evaluator of the leaf boards either way (its priors turned into the view the search turns back from)."""
    import torch
    from gymgo_amd import gogame
    N, T, L = 9, 6, 3
    roots = cs.stack(N, ('mid0', 'mid1', 'late0', 'ko', 'ended'))
    r = mc.to_dev(roots)
    hist = gogame.StoneHistory(5, N, positions=4, moves=True, device=r.device)
    kw = dict(c=1.1, komi=0.5, leaves=L, gumbel=gogame.Gumbel(4))
    a = gogame.PuctSearch(r, T, **kw)
    b = gogame.PuctSearch(r, T, features=torch.float16, symmetry=77, life=True, past=hist, **kw)
    turned = False
    for _ in range(T):
        a.backup(*pe.hash_evaluator_t(*a.select()))
        out = b.select()
        assert len(out) == 4 and out[0].dtype == torch.float16
        states = gogame.batch_untrack(b._leaf)
        p, v = pe.hash_evaluator_t(states, gogame._legal_roots(states))
        turned = turned or bool((b.orient != 0).any())
        b.backup(gogame.batch_symmetry_policy(p, b.orient), v)
    assert turned
    _same(_device_state(b), {k: mc.to_np(x) for k, x in _device_state(a).items()}, 'planes on')
    for x, y in zip(a.gumbel_root(), b.gumbel_root()):
        assert np.array_equal(pe.bits(x), pe.bits(y))


def _recording(monkeypatch):
    """Every base tensor gogame makes from here on, in order."""
    from gymgo_amd import gogame
    made, plain = [], gogame.PuctSearch._refresh_base

    def refresh(self):
        plain(self)
        made.append(mc.to_np(self.base).copy())

    monkeypatch.setattr(gogame.PuctSearch, '_refresh_base', refresh)
    return made


@pytest.mark.parametrize('reuse', [True, False])
def test_puct_play_with_gumbel(reuse, monkeypatch):
    import torch
    from gymgo_amd import gogame
    N, T, L, moves, m = 5, 4, 2, 5, 4
    A = N * N + 1
    roots = cs.stack(N, ('empty', 'mid0', 'late0', 'passed', 'ended'))
    made = _recording(monkeypatch)
    noise = lambda mv, legal: torch.from_numpy(ge.dyadic_g(5, A, mv)).to(legal.device)
    for g_dev, g_np in ((None, None), (noise, lambda mv, legal: ge.dyadic_g(5, A, mv))):
        del made[:]
        acts, final = gogame.puct_play(mc.to_dev(roots), moves, T, pe.hash_evaluator_t, komi=0.5, leaves=L, capacity=moves * T * L + 1,
                                       reuse=reuse, gumbel=m, gumbel_noise=g_dev)
        want, want_final, _ = ge.expected_play(roots, moves, T, L, pe.hash_evaluator_np, m, reuse=reuse, g_of=g_np, komi=0.5,
                                               capacity=moves * T * L + 1, base_of=lambda s: made.pop(0))
        assert not made
        assert acts.dtype == torch.int64 and np.array_equal(mc.to_np(acts), want), (reuse, g_np is not None)
        assert np.array_equal(mc.to_np(final), want_final)
        assert (want[4] == -1).all() and want[0, 0] >= 0 and want[1, 0] >= 0
    # the single-move form
    del made[:]
    got = gogame.puct_actions(mc.to_dev(roots), T, pe.hash_evaluator_t, komi=0.5, leaves=L, gumbel=m)
    s = ge.expected_gumbel(roots, T, L, pe.hash_evaluator_np, m, komi=0.5, base_of=lambda s: made.pop(0))
    assert got.dtype == torch.int64 and np.array_equal(mc.to_np(got), s.readout()[0])
    # batch_puct passes it through: the result type is unchanged, the visits are the schedule's
    del made[:]
    res = gogame.batch_puct(mc.to_dev(roots), T, pe.hash_evaluator_t, komi=0.5, leaves=L, tree=True, gumbel=m)
    st = s.state()
    assert isinstance(res, gogame.Puct) and np.array_equal(mc.to_np(res.tree.visits), st['n'])
    assert np.array_equal(pe.bits(res.tree.value_sum), pe.bits(st['w'])) and np.array_equal(mc.to_np(res.tree.parent), st['parent'])


def test_puct_selfplay_with_gumbel(monkeypatch):
    import torch
    from gymgo_amd import gogame
    N, T, L, moves, m = 5, 4, 2, 6, 4
    A = N * N + 1
    roots = cs.stack(N, ('empty', 'mid0', 'late0', 'passed', 'ended'))
    made = _recording(monkeypatch)
    noise = lambda mv, legal: torch.from_numpy(ge.dyadic_g(5, A, mv, salt=9)).to(legal.device)
    rec = gogame.puct_selfplay(mc.to_dev(roots), moves, T, pe.hash_evaluator_t, komi=0.5, leaves=L, capacity=moves * T * L + 1,
                               gumbel=gogame.Gumbel(m, None, 50.0, 0.5), gumbel_noise=noise, record_states=True)
    want = ge.expected_selfplay(roots, moves, T, L, pe.hash_evaluator_np, m, lambda mv, legal: ge.dyadic_g(5, A, mv, salt=9),
                                komi=0.5, capacity=moves * T * L + 1, base_of=lambda s: made.pop(0))
    assert not made
    assert np.array_equal(mc.to_np(rec.actions), want['actions']) and np.array_equal(mc.to_np(rec.lengths), want['lengths'])
    assert np.array_equal(pe.bits(rec.value), pe.bits(want['value']))
    assert np.array_equal(mc.to_np(rec.final_states), want['final_states'])
    pi = mc.to_np(rec.pi)
    assert pi.dtype == np.float32 and ge.ulps(pi, want['pi']).max() <= 1
    assert not pi[4].any() and (mc.to_np(rec.actions)[4] == -1).all()              # the ended game: zero rows
    live = mc.to_np(rec.actions) >= 0
    assert np.allclose(pi.astype(np.float64).sum(axis=2)[live], 1.0, atol=1e-5)
    # the default draws run, and are not bit-defined: only shapes and the legality of the moves
    rec = gogame.puct_selfplay(mc.to_dev(roots[:2]), 2, T, pe.hash_evaluator_t, komi=0.5, leaves=L, gumbel=m)
    assert tuple(rec.pi.shape) == (2, 2, A) and bool((rec.actions >= 0).all())


# ---------------------------------------------------------------- unchanged defaults
@pytest.mark.parametrize('L', [None, 3])
def test_gumbel_none_hands_out_the_parents_tree(L):
    from gymgo_amd import gogame
    N, T = 9, 10
    roots = cs.stack(N, ('mid0', 'late0', 'ko', 'ended'))
    s = gogame.PuctSearch(mc.to_dev(roots), T, c=1.1, komi=0.5, leaves=L, gumbel=None)
    assert s._gumbel is None and not hasattr(s, 'base') and not hasattr(s, '_seen') and s._L == L
    for _ in range(T):
        s.backup(*pe.hash_evaluator_t(*s.select()))
    want = (pe.expected_puct(roots, T, pe.hash_evaluator_np, c=1.1, komi=0.5) if L is None else
            pl.expected_puct_leaves(roots, T, L, pe.hash_evaluator_np, c=1.1, komi=0.5))
    pe.check(s.result(tree=True), want)
    with pytest.raises(ValueError):
        s.gumbel_root()
    with pytest.raises(ValueError):
        s.set_gumbel(np.zeros((4, N * N + 1), np.float32))


# ---------------------------------------------------------------- later trips of the grid-stride loop
B_TRIPS, TRIP_N, TRIP_ROUNDS, TRIP_L = 533, 5, 4, 3


def _trips_child():
    """533 roots of 5x5 with the library sized for one compute unit: 32 workgroups of four waves, five trips of the loop, the
    last one ragged.  Root b is root 5 b mod 11 of the size's set, so a workgroup's waves and its successive trips differ."""
    import torch
    from gymgo_amd import gogame, _lib
    assert _lib.lib().gg_device_cus() == 1
    pool = cs.stack(TRIP_N)[:11]
    idx = (5 * np.arange(B_TRIPS)) % 11
    A = TRIP_N * TRIP_N + 1
    g = ge.dyadic_g(11, A, salt=2)
    s = gogame.PuctSearch(mc.to_dev(pool[idx]), TRIP_ROUNDS, komi=0.5, leaves=TRIP_L, gumbel=4)
    s.set_gumbel(g[idx])
    bases = []
    for t in range(TRIP_ROUNDS):
        out = s.select()
        if t < 2:
            base = mc.to_np(s.base)
            assert np.array_equal(pe.bits(base), pe.bits(base[:11][np.argsort(idx[:11])][idx]))   # equal roots, equal rows
            bases.append(base[:11][np.argsort(idx[:11])].copy())
        s.backup(*pe.hash_evaluator_t(*out))
    e = ge.Search(pool, TRIP_ROUNDS, TRIP_L, 4, komi=0.5, base_of=lambda srch: bases.pop(0))
    e.set_g(g)
    for _ in range(TRIP_ROUNDS):
        e.round(pe.hash_evaluator_np)
    _same(_device_state(s), {k: v[idx] for k, v in e.state().items()}, 'trips')
    acts, pi, val = s.gumbel_root()
    w_acts, _, _, w_val, w_pi = e.readout()
    assert np.array_equal(mc.to_np(acts), w_acts[idx]) and np.array_equal(pe.bits(val), pe.bits(w_val[idx]))
    assert ge.ulps(mc.to_np(pi), w_pi[idx]).max() <= 1
    torch.cuda.synchronize()
    print('TRIPS ' + json.dumps({'ok': True, 'roots': B_TRIPS}))


def test_later_trips_of_the_grid_stride_loop():
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '1'
    assert (B_TRIPS + 3) // 4 > 4 * 32 and B_TRIPS % 4 == 1         # more than four trips of 32 workgroups, a ragged last group
    p = subprocess.run([sys.executable, os.path.abspath(__file__), 'trips'], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith('TRIPS ')][-1]
    assert json.loads(line[len('TRIPS '):]) == {'ok': True, 'roots': B_TRIPS}


if __name__ == '__main__':
    assert sys.argv[1:] == ['trips']
    _trips_child()
