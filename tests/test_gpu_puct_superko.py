"""-m gpu: positional superko at every node of a PUCT tree (k_puct_superko of gg_hash.h: gg_puct_superko,
gogame.PuctSearch(superko=history), batch_puct(superko=history), puct_play / puct_selfplay(superko='tree')), every word equal
to the definitional expectation (tests/mc_puct_superko_expect.py, which plays the children and compares positions stone by
stone; tests/test_puct_superko_host.py holds what this file relies on).

1. the launch alone at every board size 2 .. 19 on the planted cases (8 roots x 3 rows, C = 2 chunks + 2), between sentinels,
   with and without a history; the same cases tiled past one grid in a child process with the library sized for one compute
   unit; R = 0 and the argument errors in header order;
2. the search against the expectation, bit for bit, and superko=None against the plain expectation;
3. the device tree replayed on the host: no node has the stones of an ancestor or of the history;
4. tree reuse: puct_play and puct_selfplay with superko='tree', node_hash after every advance."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import hash_expect as he
import mc_expect as mc
import mc_puct_advance_expect as pa
import mc_puct_expect as pe
import mc_puct_superko_expect as se

SENTINEL32, SENTINEL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
C_PUCT, KOMI = 0.6, 0.5
BADSIZE, NULLPTR, BADARG = -1, -2, -3


def _stream():
    import torch
    from gymgo_amd import _lib
    return _lib.stream_ptr(torch.device('cuda', torch.cuda.current_device()))


def run_launch(c, tiles=1, extra_roots=0, history=True):
    """The planted case c (tiled `tiles` times, plus the first `extra_roots` roots once more) through one gg_puct_superko,
    every buffer the launch writes between sentinels -> nothing; asserts every word."""
    import torch
    from gymgo_amd import gogame, _lib
    N, C, L, H = c.N, c.C, c.L, c.H
    W = 5 * N + 1
    roots = np.concatenate([np.tile(np.arange(c.R), tiles), np.arange(extra_roots)]).astype(np.int64)
    rows = (roots[:, None] * L + np.arange(L)[None, :]).reshape(-1)
    R, B = len(roots), len(rows)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tracked = gogame.batch_track(dev(c.states[rows]))
    before = mc.to_np(tracked).copy()
    raw_leaf = torch.full((3 + B * W + 5,), SENTINEL32, dtype=torch.int32, device='cuda')
    leaf = raw_leaf[3:3 + B * W].view(B, W)
    leaf.copy_(tracked)
    raw_hash = torch.full((1 + R * (C + 1) + 3,), SENTINEL64, dtype=torch.int64, device='cuda')
    node_hash = raw_hash[1:1 + R * (C + 1)].view(R, C + 1)
    node_hash.copy_(dev(c.node_hash[roots]))
    links, move, leaf_id = dev(c.links[roots]), dev(c.move[rows]), dev(c.leaf_id[rows])
    hist, count = (dev(c.history[roots]), dev(c.count[roots])) if history else (None, None)
    _lib.call('gg_puct_superko', R, N, C, L, links, node_hash, hist, count, H if history else 0, leaf, move, leaf_id, _stream())
    if history:
        want_rows, want_hash = c.rows, c.node_hash_after
    else:
        want_rows, want_hash = se.launch(c.states, c.hashes, c.moves, c.move, c.leaf_id, c.links, c.node_hash, None, None, C, L)
    want = before.copy()
    want[:, 2 * N:3 * N] |= want_rows[rows].view(np.int32)
    got = mc.to_np(leaf)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (N, tiles, history, 'leaf', bad[:8].tolist())
    assert np.array_equal(np.delete(got, np.s_[2 * N:3 * N], axis=1), np.delete(before, np.s_[2 * N:3 * N], axis=1))
    for i in c.untouched:                                                        # skipped rows: bit for bit
        assert np.array_equal(got[rows == i], before[rows == i]), (N, c.untouched[i])
    bad = np.argwhere(mc.to_np(node_hash) != want_hash[roots])
    assert len(bad) == 0, (N, tiles, history, 'node_hash', bad[:8].tolist())
    assert bool((raw_leaf[:3] == SENTINEL32).all()) and bool((raw_leaf[3 + B * W:] == SENTINEL32).all()), (N, 'leaf sentinels')
    assert bool((raw_hash[:1] == SENTINEL64).all()) and bool((raw_hash[1 + R * (C + 1):] == SENTINEL64).all()), (N, 'hash sentinels')
    for t, w in ((links, c.links[roots]), (move, c.move[rows]), (leaf_id, c.leaf_id[rows])):     # the inputs are inputs
        assert np.array_equal(mc.to_np(t), w)


@pytest.mark.gpu
@pytest.mark.parametrize('N', range(2, 20))
def test_the_launch_alone_on_planted_cases(N):
    c = se.planted(N)
    assert c.rows.any() and (c.node_hash_after != c.node_hash).any()
    run_launch(c)
    run_launch(c, history=False)


# ---------------------------------------------------------------- later trips of the grid-stride loop
TRIP_SIZES = (6, 19)
TILES = 23          # 23 tiles of 8 roots + 1 root: 555 rows = 139 groups of four (the last holds three rows) or 278 of two (one)


def _trips_child(sizes):
    import torch
    from gymgo_amd import _lib
    assert _lib.lib().gg_device_cus() == 1
    for N in sizes:
        run_launch(se.planted(N), tiles=TILES, extra_roots=1)
    torch.cuda.synchronize()
    print('TRIPS ' + json.dumps({'sizes': list(sizes), 'ok': True}))


@pytest.mark.gpu
def test_the_launch_on_later_trips_of_its_loop():
    """More board groups than the grid: the library sized for one compute unit starts 64 workgroups, the 139 / 278 groups take
    three / five trips and the last group is ragged (tests/test_gpu_plane_trips.py's scheme)."""
    B = (TILES * se.ROOTS + 1) * se.SLOTS
    assert B == 555 and (B + 3) // 4 > 2 * 64 and B % 4 == 3 and B % 2 == 1
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '1'
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(n) for n in TRIP_SIZES], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith('TRIPS ')][-1]
    assert json.loads(line[len('TRIPS '):]) == {'sizes': list(TRIP_SIZES), 'ok': True}


@pytest.mark.gpu
def test_no_roots_and_argument_errors_in_header_order():
    import torch
    from gymgo_amd import _lib
    N, C, L, H, R = 5, 8, 2, 4, 3
    W = 5 * N + 1
    links = torch.full((R, C + 1, 2), -1, dtype=torch.int32, device='cuda')
    node_hash = torch.zeros((R, C + 2), dtype=torch.int64, device='cuda')
    history = torch.zeros((R, H + 1), dtype=torch.int64, device='cuda')
    count = torch.zeros(R + 1, dtype=torch.int32, device='cuda')
    leaf = torch.zeros((R * L, W), dtype=torch.int32, device='cuda')
    move = torch.full((R * L + 1,), -1, dtype=torch.int32, device='cuda')
    leaf_id = torch.full((R * L + 1,), -1, dtype=torch.int32, device='cuda')
    fn, s = _lib.lib().gg_puct_superko, _stream()
    p = lambda t, off=0: t.data_ptr() + off
    good = dict(R=R, N=N, C=C, L=L, links=p(links), node_hash=p(node_hash), history=p(history), count=p(count), H=H, leaf=p(leaf),
                move=p(move), leaf_id=p(leaf_id))
    call = lambda **kw: fn(*[{**good, **kw}[k] for k in good], s)
    assert call() == 0
    assert call(R=0) == 0 and call(R=0, links=None, leaf=None) == 0                  # no roots: no work, before the pointers
    assert call(history=None, count=None) == 0 and call(history=None, count=None, H=7) == 0
    for kw in (dict(N=1), dict(N=20), dict(R=-1)):
        assert call(**kw) == BADSIZE, kw
    for kw in (dict(C=0), dict(C=2 ** 31 - 1), dict(L=0), dict(L=C + 1), dict(H=-1)):
        assert call(**kw) == BADARG, kw
    for name in ('links', 'node_hash', 'leaf', 'move', 'leaf_id'):
        assert call(**{name: None}) == NULLPTR, name
    assert call(history=None) == NULLPTR and call(count=None) == NULLPTR             # exactly one of the pair
    for kw in (dict(node_hash=p(node_hash, 4)), dict(history=p(history, 4)), dict(links=p(links, 2)), dict(count=p(count, 2)),
               dict(leaf=p(leaf, 1)), dict(move=p(move, 2)), dict(leaf_id=p(leaf_id, 3))):
        assert call(**kw) == BADARG, kw
    # the order of the header: size before argument before R = 0 before pointer before alignment
    assert call(N=1, C=0, links=None) == BADSIZE and call(R=-1, L=0) == BADSIZE
    assert call(C=0, R=0) == BADARG and call(H=-1, leaf=None) == BADARG
    assert call(R=0, node_hash=p(node_hash, 4)) == 0
    assert call(links=None, node_hash=p(node_hash, 4)) == NULLPTR
    torch.cuda.synchronize()
    assert not bool(leaf.any()) and not bool(node_hash.any())                       # all rows were skipped rows


# ---------------------------------------------------------------- 2. and 3.: the search
def roots7(N, seed=60):
    roots = mc.make_roots(N, 7, seed + N, max_ply=N * N, step=1)
    assert roots.shape[0] == 7 and roots[-1, 5, 0, 0] == 1
    return roots


def recorded(roots):
    """Per root a game record for the search to respect: an invented earlier position - the child of the root's last candidate,
    as if the game had been there - and the root itself -> (boards per root, history int64 [R, 3], count int32 [R])."""
    from oracle import c_oracle
    import outcome_expect as oe
    N = roots.shape[-1]
    boards, hist, count = [], np.zeros((len(roots), 3), np.int64), np.zeros(len(roots), np.int32)
    for r, s in enumerate(roots):
        cand = np.flatnonzero(oe.candidates(s).reshape(-1))
        mine = ([c_oracle.next_state(s, int(cand[-1]))] if len(cand) else []) + [s]
        boards.append(mine)
        hist[r, :len(mine)], count[r] = [he.hash_of(b) for b in mine], len(mine)
    return boards, hist, count


def history_of(hist, count):
    import torch
    from gymgo_amd import gogame
    h = gogame.PositionHistory(hist.shape[0], hist.shape[1])
    h.hashes.copy_(torch.from_numpy(hist))
    h.count.copy_(torch.from_numpy(count))
    return h


def evaluators(name):
    """(the expectation's evaluator of states, the device's evaluator, the features dtype)"""
    import torch
    import test_gpu_symmetry_io as tsio
    if name == 'hash':
        return pe.hash_evaluator_np, pe.hash_evaluator_t, None
    if name == 'pass':
        return pe.pass_evaluator_np, pe.pass_evaluator_t, None
    return se.planes_evaluator(tsio.point_evaluator), tsio.on_device(tsio.point_evaluator), torch.float16


def replayed(roots, r, parent, action, nodes):
    """The tree of root r rebuilt on the host from (parent, action) alone with the C restatement, as se.repeats takes it."""
    from oracle import c_oracle
    N = roots.shape[-1]
    boards = [roots[r]]
    for y in range(1, int(nodes)):
        s = boards[int(parent[y])].copy()
        s[3] = 0                                                   # (the marks are not the game's: play by the stones)
        boards.append(c_oracle.next_state(s, int(action[y])))
    return SimpleNamespace(boards=boards, parent=parent, action=action, prior=np.zeros((1, N * N + 1)))


@pytest.mark.gpu
@pytest.mark.parametrize('N,I,name', [(2, 64, 'hash'), (3, 200, 'pass'), (2, 64, 'point'), (3, 200, 'point')])
@pytest.mark.parametrize('leaves', (None, 2))
def test_the_search_against_the_expectation(N, I, name, leaves):
    from gymgo_amd import gogame
    roots = roots7(N)
    E_np, E_dev, feat = evaluators(name)
    boards, hist, count = recorded(roots)
    kw = dict(c=C_PUCT, komi=KOMI, leaves=leaves)
    want = se.expected_puct(roots, boards, I, E_np, **kw)
    plain = se.expected_puct(roots, None, I, E_np, rule=False, **kw)
    assert sum(len(a) for t in want['trees'] for y, a in t.marks.items() if y > 0) > 0     # the rule acts below the root
    st = mc.to_dev(roots)
    got = gogame.batch_puct(st, I, E_dev, tree=True, features=feat, superko=history_of(hist, count), **kw)
    pe.check(got, want, tag=(N, name, leaves, 'superko'))
    none = gogame.batch_puct(st, I, E_dev, tree=True, features=feat, superko=None, **kw)
    pe.check(none, plain, tag=(N, name, leaves, 'superko=None'))
    pe.check(gogame.batch_puct(st, I, E_dev, tree=True, features=feat, **kw), plain, tag=(N, name, leaves, 'default'))
    # 3. the device trees replayed from (parent, action): no node has the stones of an ancestor or of the record
    parent, action, nodes = (mc.to_np(x) for x in (got.tree.parent, got.tree.action, got.nodes))
    for r in range(len(roots)):
        t = replayed(roots, r, parent[r], action[r], nodes[r])
        assert not se.repeats(t, {se.key_of(b) for b in boards[r]}), (N, name, leaves, r)
    parent, action, nodes = (mc.to_np(x) for x in (none.tree.parent, none.tree.action, none.nodes))
    n = [len(se.repeats(replayed(roots, r, parent[r], action[r], nodes[r]))) for r in range(len(roots))]
    assert n == [len(se.repeats(t)) for t in plain['trees']], (N, name, leaves)
    assert sum(n) > 0 or (N, name, leaves) == (3, 'point', None)   # the premise: the same search without the rule has such nodes
    if leaves is None and name != 'point':
        import test_puct_superko_host as host
        assert tuple(n) == host.COUNTS[(N, name, I)]


@pytest.mark.gpu
def test_the_search_refuses_a_history_on_another_device():
    import torch
    from gymgo_amd import gogame
    st = torch.zeros((2, 6, 3, 3), dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='history'):
        gogame.PuctSearch(st, 4, superko=gogame.PositionHistory(2, 4, device='cpu'))
    search = gogame.PuctSearch(st, 4)
    with pytest.raises(ValueError, match='history'):
        search.forbid_repeats()                                      # no history of its own, none given


# ---------------------------------------------------------------- 4. reuse
M_PLAY, T_PLAY = 24, 4


def play_kw():
    import torch
    return dict(c=C_PUCT, komi=KOMI, leaves=2, capacity=512, features=torch.float16)


@pytest.mark.gpu
@pytest.mark.parametrize('N', (2, 3))
def test_selfplay_on_the_ruled_tree(N):
    import test_gpu_features as tgf
    import test_gpu_hash as tgh
    import test_gpu_symmetry_io as tsio
    from gymgo_amd import gogame
    roots = roots7(N, seed=90)
    st = mc.to_dev(roots)
    E = tsio.on_device(tsio.point_evaluator)
    kw = dict(record_states=True, seed=7, **play_kw())
    got = gogame.puct_selfplay(st, M_PLAY, T_PLAY, E, superko='tree', **kw)
    want = se.expected_selfplay(roots, M_PLAY, T_PLAY, se.planes_evaluator(tsio.point_evaluator), c=C_PUCT, komi=KOMI, leaves=2,
                                capacity=512, seed=7)
    for k in ('actions', 'lengths', 'outcome', 'states', 'final_states', 'pi', 'value'):
        g, w = mc.to_np(getattr(got, k)), want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (N, k, g.dtype, w.dtype)
        assert np.array_equal(pe.bits(g), pe.bits(w)), (N, k, np.argwhere(pe.bits(g) != pe.bits(w))[:8])
    assert not tgh.recreations(mc.to_np(got.states), mc.to_np(got.actions), mc.to_np(got.final_states)), N
    tgf.same_tuples(gogame.puct_selfplay(st, M_PLAY, T_PLAY, E, superko=False, **kw), gogame.puct_selfplay(st, M_PLAY, T_PLAY, E, **kw), N)
    with pytest.raises(ValueError, match='superko'):
        gogame.puct_selfplay(st, M_PLAY, T_PLAY, E, superko='roots', **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('N', (2, 3))
@pytest.mark.parametrize('reuse', (True, False))
def test_play_on_the_ruled_tree(N, reuse):
    import torch
    import test_gpu_symmetry_io as tsio
    from gymgo_amd import gogame
    from oracle import c_oracle
    roots = roots7(N, seed=90)
    st = mc.to_dev(roots)
    E = tsio.on_device(tsio.point_evaluator)
    acts, final = gogame.puct_play(st, M_PLAY, T_PLAY, E, reuse=reuse, superko='tree', **play_kw())
    want_acts, want_final, _ = se.expected_puct_play(roots, M_PLAY, T_PLAY, se.planes_evaluator(tsio.point_evaluator), c=C_PUCT,
                                                      komi=KOMI, leaves=2, capacity=512, reuse=reuse)
    assert np.array_equal(mc.to_np(acts), want_acts), (N, reuse, np.argwhere(mc.to_np(acts) != want_acts)[:8])
    assert np.array_equal(mc.to_np(final), want_final), (N, reuse)
    acts = mc.to_np(acts)
    for r in range(len(roots)):                                     # no move played recreates a position
        cur, keys = roots[r].copy(), {se.key_of(roots[r])}
        for a in acts[r]:
            if a < 0:
                continue
            cur[3] = 0
            cur = c_oracle.next_state(cur, int(a))
            assert a == N * N or se.key_of(cur) not in keys, (N, reuse, r)
            keys.add(se.key_of(cur))
    a = gogame.puct_play(st, 6, T_PLAY, E, reuse=reuse, superko=False, **play_kw())
    b = gogame.puct_play(st, 6, T_PLAY, E, reuse=reuse, **play_kw())
    assert all(torch.equal(x, y) for x, y in zip(a, b)), (N, reuse)
    with pytest.raises(ValueError, match='superko'):
        gogame.puct_play(st, 6, T_PLAY, E, reuse=reuse, superko='roots', **play_kw())


@pytest.mark.gpu
@pytest.mark.parametrize('N', (2, 3))
def test_node_hash_follows_the_tree_through_rounds_and_advances(N):
    """The move loop by hand on PuctSearch(superko=history): after every move's rounds and after every advance node_hash of the
    nodes in use is batch_hash_tracked of their boards, and the trees are the expectation's."""
    import torch
    import test_gpu_symmetry_io as tsio
    from gymgo_amd import gogame
    roots = roots7(N, seed=90)
    st = mc.to_dev(roots)
    R, L, NN, M = len(roots), 2, 96, 8
    E_np, E = se.planes_evaluator(tsio.point_evaluator), tsio.on_device(tsio.point_evaluator)
    history = gogame.PositionHistory(R, M + 1)
    search = gogame.PuctSearch(st, T_PLAY, c=C_PUCT, komi=KOMI, leaves=L, capacity=NN, features=torch.float16, superko=history)
    history.push(search._root_hashes())
    trees = se.make_trees(roots, None, NN, L)

    def hashes_hold(tag):
        nodes = mc.to_np(search.result().nodes)
        want = mc.to_np(gogame.batch_hash_tracked(search._boards.view(R * NN, -1))).reshape(R, NN)
        got = mc.to_np(search.node_hash)
        for r in range(R):
            assert np.array_equal(got[r, :nodes[r]], want[r, :nodes[r]]), (N, tag, r)
        assert got.any()

    hashes_hold('begin')
    for mv in range(M):
        search.forbid_repeats()
        for t in trees:
            t.forbid_root()
        for _ in range(T_PLAY):
            search.backup(*E(*search.select()))
        pa.search_rounds(trees, T_PLAY, L, E_np, C_PUCT, KOMI)
        hashes_hold(('rounds', mv))
        pe.check(search.result(tree=True), pa.results(trees, N * N + 1), tag=(N, mv))
        acts = [pa.most_visited_root(t) for t in trees]
        kept = search.advance(np.array(acts, np.int64))
        assert mc.to_np(kept).tolist() == [se.advance(t, a) for t, a in zip(trees, acts)], (N, mv)
        history.push(search._root_hashes())
        hashes_hold(('advance', mv))


if __name__ == '__main__':
    _trips_child([int(a) for a in sys.argv[1:]])
