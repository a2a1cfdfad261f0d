"""-m gpu: PUCT tree search (gogame.batch_puct / PuctSearch: gg_puct_begin / k_puct_select / the tracked one-move step / untrack
/ the caller's evaluator / k_puct_backup) - every Puct field and the whole tree equal to the restatement
(tests/mc_puct_expect.py) exactly, value sums as bit patterns: ended nodes inside the tree, every board size class, komi,
crafted roots, c = 0 and a large c, hostile evaluator outputs, the playout evaluator under both policies, the step-wise form,
NumPy input, shards by root, a non-default stream, R = 0, the roots unmodified."""
import math

import numpy as np
import pytest

import mc_expect as mc
import mc_puct_expect as pe

pytestmark = pytest.mark.gpu


def _invariants(got, I):
    legal = mc.to_np(got.legal)
    live = legal.any(axis=1)
    v = mc.to_np(got.visits)
    assert (mc.to_np(got.root_visits) == I).all()
    assert (v.sum(axis=1)[live] == I - 1).all() and not v[~legal].any() and not mc.to_np(got.priors)[~legal].any()


def test_puct_5x5_revisits_ended_nodes():
    """I far past the root's 26 actions: nodes whose game has ended (a pass after a pass) lie inside the tree, are scored on
    the device and evaluated again each time the walk reaches them; NumPy in, NumPy out."""
    from gymgo_amd import gogame
    N, I = 5, 200
    roots = np.concatenate([mc.crafted_roots(N)[:3], mc.make_roots(N, 4, 31, max_ply=20, step=6)[1:3]])
    want = pe.expected_puct(roots, I, pe.hash_evaluator_np, c=0.6, komi=0.5)
    revisited = sum(1 for t in want['trees'] for x in range(1, len(t.boards)) if t.legal[x].size == 0 and t.n[x] > 1)
    assert revisited > 0
    got = gogame.batch_puct(roots, I, pe.hash_evaluator_t, c=0.6, komi=0.5, tree=True)
    assert isinstance(got.visits, np.ndarray) and got.visits.dtype == np.int32 and got.value_sum.dtype == np.float64
    assert got.priors.dtype == np.float32 and got.legal.dtype == np.bool_ and got.tree.value_sum.dtype == np.float64
    pe.check(got, want)
    _invariants(got, I)


@pytest.mark.parametrize('N', [7, 9])
def test_puct_mid_game_and_crafted_roots(N):
    import torch
    from gymgo_amd import gogame
    I = 2 * N * N
    roots = np.concatenate([mc.make_roots(N, 4, 50 + N, max_ply=N * N, step=N)[1:3], mc.crafted_roots(N)])
    want = pe.expected_puct(roots, I, pe.hash_evaluator_np, komi=0.5)
    r = mc.to_dev(roots)
    before = r.clone()
    got = gogame.batch_puct(r, I, pe.hash_evaluator_t, komi=0.5, tree=True)
    assert got.legal.dtype == torch.bool and got.visits.dtype == torch.int32 and got.value_sum.dtype == torch.float64
    assert got.priors.dtype == torch.float32 and got.nodes.dtype == torch.int32
    pe.check(got, want)
    assert bool((r == before).all())                                  # the roots are not modified
    _invariants(got, I)
    ko = roots.shape[0] - 2
    assert not mc.to_np(got.legal)[ko, mc.KO_POINT[0] * N + mc.KO_POINT[1]]
    # the ended root: no node but itself, evaluated I times with its own outcome; the root after one pass: live
    assert mc.to_np(got.nodes)[-1] == 1 and not mc.to_np(got.legal)[-1].any() and abs(float(got.root_value_sum[-1])) in (0.0, float(I))
    assert np.array_equal(mc.to_np(gogame.puct_actions(r, I, pe.hash_evaluator_t, komi=0.5)), pe.most_visited(want))
    assert pe.most_visited(want)[-1] == -1


def test_puct_13x13():
    from gymgo_amd import gogame
    N, I = 13, 120
    roots = np.concatenate([mc.make_roots(N, 4, 13, max_ply=150, step=50)[1:], mc.crafted_roots(N)[1:3]])
    want = pe.expected_puct(roots, I, pe.hash_evaluator_np, c=2.0, komi=6.5)
    got = gogame.batch_puct(mc.to_dev(roots), I, pe.hash_evaluator_t, c=2.0, komi=6.5, tree=True)
    pe.check(got, want)
    _invariants(got, I)


@pytest.mark.parametrize('komi', [7.5, 0.0])
def test_puct_19x19(komi):
    from gymgo_amd import gogame
    N, I = 19, 60
    roots = np.concatenate([mc.make_roots(N, 4, 7, max_ply=240, step=120)[1:], mc.crafted_roots(N)[1:]])
    want = pe.expected_puct(roots, I, pe.hash_evaluator_np, komi=komi)
    got = gogame.batch_puct(mc.to_dev(roots), I, pe.hash_evaluator_t, komi=komi, tree=True)
    pe.check(got, want, tag=komi)
    _invariants(got, I)
    one = gogame.puct(mc.to_dev(roots[1]), I, pe.hash_evaluator_t, komi=komi, tree=True)
    for k in pe.ROOT_KEYS:
        assert np.array_equal(pe.bits(getattr(one, k)), pe.bits(want[k][1])), k
    for k in pe.TREE_KEYS:
        assert np.array_equal(pe.bits(getattr(one.tree, k)), pe.bits(want['tree'][k][1])), k


def test_puct_ended_root_and_root_after_one_pass():
    """The ended roots of every size class are scored by the device's own floods (komi decides a drawn board); the root after
    one pass has a pass child whose game has ended."""
    from gymgo_amd import gogame
    for N, komi in ((5, 0.0), (9, -0.5), (13, 0.5), (19, 7.5)):
        full = mc.make_roots(N, 2, 3 + N, max_ply=8, step=8)[-1:]               # a game played to its end
        roots = np.concatenate([mc.crafted_roots(N)[3:], full, mc.crafted_roots(N)[1:2]])
        I = 40
        want = pe.expected_puct(roots, I, pe.hash_evaluator_np, komi=komi)
        got = gogame.batch_puct(mc.to_dev(roots), I, pe.hash_evaluator_t, komi=komi, tree=True)
        pe.check(got, want, tag=N)
        assert got.nodes.tolist()[:2] == [1, 1] and got.root_visits.tolist() == [I] * 3
        assert abs(float(got.root_value_sum[0])) == (0.0 if komi == 0.0 else float(I))
        # all the prior on the pass: the first selection below the root after one pass plays it, the child has ended
        want = pe.expected_puct(roots[2:], I, pe.pass_evaluator_np, komi=komi)
        t = want['trees'][0]
        assert t.action[1] == N * N and t.legal[1].size == 0 and t.n[1] >= 1
        pe.check(gogame.batch_puct(mc.to_dev(roots[2:]), I, pe.pass_evaluator_t, komi=komi, tree=True), want, tag=(N, 'pass'))


@pytest.mark.parametrize('c', [0.0, 1e6])
def test_puct_c_zero_and_large(c):
    from gymgo_amd import gogame
    N, I = 9, 150
    roots = mc.make_roots(N, 6, 62, max_ply=80, step=16)
    want = pe.expected_puct(roots, I, pe.hash_evaluator_np, c=c, komi=0.5)
    got = gogame.batch_puct(mc.to_dev(roots), I, pe.hash_evaluator_t, c=c, komi=0.5, tree=True)
    pe.check(got, want, tag=c)
    _invariants(got, I)


@pytest.mark.parametrize('c', [1.25, 0.0])
def test_puct_hostile_evaluator(c):
    """NaN, negative and infinite priors, mass on illegal actions, all-zero rows; values outside [-1, 1], NaN, infinite: the
    stored priors are finite-or-inf, non-negative and zero on illegal actions, every w is finite, the tree is the
    restatement's.  c = 0 with an infinite prior makes U a NaN, which counts as -inf."""
    from gymgo_amd import gogame
    N, I = 9, 150
    roots = np.concatenate([mc.make_roots(N, 6, 77, max_ply=60, step=12), mc.crafted_roots(N)])
    want = pe.expected_puct(roots, I, pe.hostile_evaluator_np, c=c, komi=0.5)
    stored = np.stack([t.prior for t in want['trees']])
    assert np.isposinf(stored).any() and (stored >= 0).all()
    got = gogame.batch_puct(mc.to_dev(roots), I, pe.hostile_evaluator_t, c=c, komi=0.5, tree=True)
    pe.check(got, want, tag=c)
    _invariants(got, I)
    assert np.isfinite(mc.to_np(got.tree.value_sum)).all() and (np.abs(mc.to_np(got.tree.value_sum)) <= I).all()
    pr = mc.to_np(got.priors)
    assert not np.isnan(pr).any() and (pr >= 0).all()


@pytest.mark.parametrize('policy', ['uniform', 'no_eye_fill'])
def test_puct_playout_evaluator(policy):
    import torch
    from gymgo_amd import gogame
    N, I, K, f0 = 9, 30, 8, 2
    roots = np.concatenate([mc.make_roots(N, 4, 5, max_ply=60, step=20)[1:], mc.crafted_roots(N)[1:]])
    want = pe.expected_puct(roots, I, pe.playout_evaluator_np(K, 672, komi=0.5, seed=11, first_root=f0, policy=policy), komi=0.5)
    ev = gogame.playout_evaluator(K, seed=11, first_root=f0, policy=policy, slots=64, komi=0.5)
    got = gogame.batch_puct(mc.to_dev(roots), I, ev, komi=0.5, tree=True)
    pe.check(got, want, tag=policy)
    # its outputs on their own: uniform over the legal actions, (wins - losses) / K of batch_playouts with call 0's seed
    ev = gogame.playout_evaluator(K, seed=11, first_root=f0, policy=policy, komi=0.5)
    st = mc.to_dev(roots)
    legal = torch.from_numpy(mc.legal_mask(roots)).cuda()
    p, v = ev(st, legal)
    wp, wv = pe.playout_evaluator_np(K, 672, komi=0.5, seed=11, first_root=f0, policy=policy)(roots, mc.legal_mask(roots))
    assert p.dtype == torch.float32 and v.dtype == torch.float32
    assert np.array_equal(pe.bits(p), pe.bits(wp)) and np.array_equal(pe.bits(v), pe.bits(wv))


def test_puct_search_step_by_step_numpy_input_shards_and_stream():
    import torch
    from gymgo_amd import gogame
    N, I, R = 9, 60, 7
    roots = mc.make_roots(N, R, 41, max_ply=70, step=10)
    want = pe.expected_puct(roots, I, pe.hash_evaluator_np, c=1.1, komi=0.5)
    r = mc.to_dev(roots)
    whole = gogame.batch_puct(r, I, pe.hash_evaluator_t, c=1.1, komi=0.5, tree=True)
    pe.check(whole, want, tag='whole')
    # the step-wise form, with partial results on the way and the call order enforced
    s = gogame.PuctSearch(r, I, c=1.1, komi=0.5)
    with pytest.raises(ValueError):
        s.backup(torch.zeros((R, N * N + 1), device='cuda'), torch.zeros(R, device='cuda'))
    for i in range(I):
        states, legal = s.select()
        assert states.is_cuda and states.dtype == torch.uint8 and tuple(states.shape) == (R, 6, N, N)
        assert legal.is_cuda and legal.dtype == torch.bool and tuple(legal.shape) == (R, N * N + 1)
        if i == 0:
            assert bool((states == r).all())                          # iteration 0 hands out the roots
            with pytest.raises(ValueError):
                s.select()
            with pytest.raises(ValueError):
                s.result()
        assert np.array_equal(mc.to_np(legal), mc.legal_mask(mc.to_np(states)))
        s.backup(*pe.hash_evaluator_t(states, legal))
        if i == 9:
            pe.check(s.result(tree=True), pe.expected_puct(roots, 10, pe.hash_evaluator_np, c=1.1, komi=0.5)
                     | {'tree': _padded_tree(roots, 10, I)}, tag='partial')
    with pytest.raises(ValueError):
        s.select()
    pe.check(s.result(tree=True), want, tag='steps')
    pe.check(s.result(), want, tree=False, tag='steps')
    # NumPy evaluations into backup; NumPy roots
    s = gogame.PuctSearch(roots, I, c=1.1, komi=0.5)
    for i in range(I):
        states, legal = s.select()
        assert states.is_cuda
        s.backup(*pe.hash_evaluator_np(mc.to_np(states), mc.to_np(legal)))
    got = s.result(tree=True)
    assert isinstance(got.visits, np.ndarray)
    pe.check(got, want, tag='numpy')
    pe.check(gogame.batch_puct(roots, I, pe.hash_evaluator_t, c=1.1, komi=0.5, tree=True), want, tag='numpy roots')
    # shards by root concatenate to the whole
    a = gogame.batch_puct(r[:3], I, pe.hash_evaluator_t, c=1.1, komi=0.5)
    b = gogame.batch_puct(r[3:], I, pe.hash_evaluator_t, c=1.1, komi=0.5)
    pe.check(gogame.Puct(*[torch.cat([x, y]) for x, y in zip(a[:-1], b[:-1])], tree=None), want, tree=False, tag='shards')
    # a non-default stream
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = gogame.batch_puct(r, I, pe.hash_evaluator_t, c=1.1, komi=0.5, tree=True)
    stream.synchronize()
    pe.check(got, want, tag='stream')
    assert bool((r == mc.to_dev(roots)).all())


def _padded_tree(roots, done, I):
    """The tree fields after `done` iterations of a search with room for I + 1 nodes."""
    e = pe.expected_puct(roots, done, pe.hash_evaluator_np, c=1.1, komi=0.5)['tree']
    out = {}
    for k in pe.TREE_KEYS:
        fill = -1 if k in ('parent', 'action') else 0
        out[k] = np.concatenate([e[k], np.full((e[k].shape[0], I - done), fill, e[k].dtype)], axis=1)
    return out


def test_puct_empty_batch_and_argument_errors():
    import torch
    from gymgo_amd import gogame
    N = 9
    calls = []

    def ev(states, legal):
        calls.append((tuple(states.shape), tuple(legal.shape)))
        return torch.zeros((0, N * N + 1), device='cuda'), torch.zeros(0, device='cuda')

    got = gogame.batch_puct(torch.zeros((0, 6, N, N), dtype=torch.uint8, device='cuda'), 3, ev, tree=True)
    assert calls == [((0, 6, N, N), (0, N * N + 1))] * 3
    assert got.legal.shape == (0, N * N + 1) and got.nodes.shape == (0,) and got.tree.parent.shape == (0, 4)
    assert got.value_sum.dtype == torch.float64 and got.tree.value_sum.shape == (0, 4)
    assert gogame.puct_actions(torch.zeros((0, 6, N, N), dtype=torch.uint8, device='cuda'), 3, ev).shape == (0,)
    roots = mc.to_dev(mc.make_roots(N, 2, 3, max_ply=20, step=10))
    for bad in (dict(iterations=0), dict(c=-1.0), dict(c=math.inf), dict(c=math.nan), dict(komi=math.nan)):
        kw = dict(iterations=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            gogame.batch_puct(roots, evaluator=pe.hash_evaluator_t, **kw)
    s = gogame.PuctSearch(roots, 2)
    s.select()
    with pytest.raises(ValueError):
        s.backup(torch.zeros((2, 5), device='cuda'), torch.zeros(2, device='cuda'))
    ended = np.repeat(mc.crafted_roots(N)[3:], 3, axis=0)
    assert gogame.puct_actions(mc.to_dev(ended), 4, pe.hash_evaluator_t).tolist() == [-1, -1, -1]


def test_puct_select_without_room_evaluates_the_node_it_stopped_at():
    """I iterations use I of a tree's I + 1 nodes.  PuctSearch refuses further selects on the host, so the entry points are
    called directly on the search's buffers: select I + 1 takes the last node, every select after that finds no room where
    it wants to expand - it hands out the node it stopped at with move = -1 and writes nothing beyond the tree - and the
    backup counts the visit.  Leaf id, move, leaf board and the whole tree equal the restatement after each extra iteration."""
    import torch
    from gymgo_amd import gogame, _lib
    N, I, c, komi, extra = 5, 12, 0.6, 0.5, 6
    A, W = N * N + 1, 5 * N + 1
    roots = np.concatenate([mc.crafted_roots(N)[:3], mc.make_roots(N, 5, 23, max_ply=20, step=5)[1:4]])
    R = roots.shape[0]
    want = pe.expected_puct(roots, I, pe.hash_evaluator_np, c=c, komi=komi)
    trees = want['trees']
    s = gogame.PuctSearch(mc.to_dev(roots), I, c=c, komi=komi)
    for _ in range(I):
        s.backup(*pe.hash_evaluator_t(*s.select()))
    pe.check(s.result(tree=True), want)
    assert s._nodes.tolist() == [len(t.boards) for t in trees]
    L, stream = _lib.lib(), _lib.current_raw_stream(torch.device('cuda', torch.cuda.current_device()))
    boards, child, prior, links, stats, nodes = s._tree
    lp, mp, ip = s._out
    states = torch.empty((R, 6, N, N), dtype=torch.uint8, device='cuda')
    no_room = 0
    for k in range(extra):
        assert L.gg_puct_select(R, N, I, c, boards, child, prior, links, stats, nodes, lp, mp, ip, stream) == 0
        picked = [t.select(c) for t in trees]
        full = [len(t.boards) == I + 1 for t in trees]
        ids, moves = [t.paths[-1][0] for t in trees], [t.paths[-1][1] for t in trees]
        assert s._leaf_id.tolist() == ids and s._move.tolist() == moves, k
        no_room += sum(1 for r, t in enumerate(trees) if k > 0 and full[r] and moves[r] == -1 and t.legal[ids[r]].size
                       and t.n[ids[r]] > 0)
        assert L.gg_batch_play_moves_tracked(lp, mp, None, R, N, 1, stream) == 0
        assert L.gg_batch_untrack_states(lp, states.data_ptr(), R, N, stream) == 0
        leaves = np.stack([b for _, b in picked])
        assert np.array_equal(mc.to_np(states), leaves), k
        legal = torch.from_numpy(mc.legal_mask(leaves)).cuda()
        p, v = pe.hash_evaluator_t(states, legal)
        assert L.gg_puct_backup(R, N, I, komi, p.contiguous().data_ptr(), v.contiguous().data_ptr(), boards, prior, links, stats,
                                lp, mp, ip, stream) == 0
        pn, vn = pe.hash_evaluator_np(leaves, mc.legal_mask(leaves))
        for r, t in enumerate(trees):
            t.backup(ids[r], pn[r], vn[r], komi)
        assert (s._nodes <= I + 1).all() and s._nodes.tolist() == [len(t.boards) for t in trees]
        assert np.array_equal(mc.to_np(s._child), np.stack([t.child for t in trees]).astype(np.int32)), k
        assert np.array_equal(mc.to_np(s._links[..., 0]), np.stack([t.parent for t in trees])), k
        assert np.array_equal(mc.to_np(s._stats[..., 2]), np.stack([t.n for t in trees])), k
        assert np.array_equal(pe.bits(s._stats.view(torch.float64)[..., 0]), pe.bits(np.stack([t.w for t in trees]))), k
        assert np.array_equal(pe.bits(s._prior), pe.bits(np.stack([t.prior for t in trees]))), k
    assert no_room > 0                              # the branch was taken, at live and evaluated nodes
    assert all(t.n[0] == I + extra for t in trees)


@pytest.mark.parametrize('N', [5, 9])
def test_puct_one_leaf_entry_points_ignore_the_reserved_word(N):
    """gg_puct_select / gg_puct_backup on this test's own buffers, I iterations from an ended root, a root after a pass and a
    mid-game root: once with the reserved word of every stat record at 0, once at 7.  Every tree buffer but that word is the
    same bytes in both runs and equal to the restatement, and the word is still 7 on every record afterwards - the one-leaf
    kernels neither read nor write it."""
    import torch
    from gymgo_amd import gogame, _lib
    I, c, komi = 12, 0.6, 0.5
    A, W, NN = N * N + 1, 5 * N + 1, I + 1
    roots = np.concatenate([mc.crafted_roots(N)[3:], mc.crafted_roots(N)[1:2], mc.make_roots(N, 4, 29 + N, max_ply=3 * N, step=N)[2:3]])
    R = roots.shape[0]
    assert R == 3 and roots[0, 5].all() and roots[1, 4].all() and not roots[1:, 5].any() and roots[2, :2].any()
    want = pe.expected_puct(roots, I, pe.hash_evaluator_np, c=c, komi=komi)
    dev = torch.device('cuda', torch.cuda.current_device())
    lib, stream = _lib.lib(), _lib.current_raw_stream(dev)
    tracked = gogame._track_roots(mc.to_dev(roots))

    def run(word):
        z = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype, device=dev)
        t = dict(boards=z(R, NN, W), child=z(R, NN, A), prior=z(R, NN, A, dtype=torch.float32), links=z(R, NN, 2),
                 stats=z(R, NN, 4), nodes=z(R))
        leaf, move, leaf_id = z(R, W), z(R), z(R)
        states = torch.empty((R, 6, N, N), dtype=torch.uint8, device=dev)
        tree = [t[k].data_ptr() for k in ('boards', 'child', 'prior', 'links', 'stats', 'nodes')]
        out = [leaf.data_ptr(), move.data_ptr(), leaf_id.data_ptr()]
        assert lib.gg_puct_begin(tracked.data_ptr(), R, N, I, *tree, stream) == 0
        t['stats'][..., 3] = word
        for _ in range(I):
            assert lib.gg_puct_select(R, N, I, c, *tree, *out, stream) == 0
            assert lib.gg_batch_play_moves_tracked(out[0], out[1], None, R, N, 1, stream) == 0
            assert lib.gg_batch_untrack_states(out[0], states.data_ptr(), R, N, stream) == 0
            p, v = pe.hash_evaluator_t(states, gogame._legal_roots(states))
            assert lib.gg_puct_backup(R, N, I, komi, p.contiguous().data_ptr(), v.contiguous().data_ptr(), t['boards'].data_ptr(),
                                      t['prior'].data_ptr(), t['links'].data_ptr(), t['stats'].data_ptr(), *out, stream) == 0
        assert bool((t['stats'][..., 3] == word).all())                # the word is where it was, on every record
        return t

    a, b = run(0), run(7)
    for k in ('boards', 'child', 'links', 'nodes'):
        assert bool((a[k] == b[k]).all()), k
    assert bool((a['prior'].view(torch.int32) == b['prior'].view(torch.int32)).all())
    assert bool((a['stats'][..., :3] == b['stats'][..., :3]).all())
    trees = want['trees']
    assert b['nodes'].tolist() == [len(t.boards) for t in trees]
    assert np.array_equal(mc.to_np(b['child']), np.stack([t.child for t in trees]).astype(np.int32))
    assert np.array_equal(mc.to_np(b['links'][..., 0]), np.stack([t.parent for t in trees]))
    assert np.array_equal(mc.to_np(b['links'][..., 1]), np.stack([t.action for t in trees]))
    assert np.array_equal(mc.to_np(b['stats'][..., 2]), np.stack([t.n for t in trees]))
    assert np.array_equal(pe.bits(b['stats'].view(torch.float64)[..., 0]), pe.bits(np.stack([t.w for t in trees])))
    assert np.array_equal(pe.bits(b['prior']), pe.bits(np.stack([t.prior for t in trees])))
    for r, t in enumerate(trees):   # the boards of the nodes in use
        assert np.array_equal(mc.to_np(gogame.batch_untrack(b['boards'][r, :len(t.boards)].contiguous())), np.stack(t.boards)), r
