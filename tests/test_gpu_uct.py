"""-m gpu: UCT tree search (gogame.batch_uct: gg_uct_begin / k_uct_select / the tracked one-move step / the playout queue /
k_uct_backup) - every Uct field and the whole tree equal to the restatement (tests/mc_expect.py) bit for bit: terminal nodes
inside the tree, crafted roots (empty board, pass root, active ko, ended root), 19x19 with komi and first_root, all three
rollout families under the leaf playouts, invariance under the slot count, the chunk length and sharding by root;
uct_actions."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import mc_expect as mc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _check(got, want, tree=False, tag=''):
    mc.check(got, want, mc.ROOT_KEYS, tag)
    if tree:
        mc.check(got.tree, want['tree'], mc.TREE_KEYS, (tag, 'tree'))
    else:
        assert got.tree is None


def _invariants(got, roots, I, K):
    legal = mc.to_np(got.legal)
    live = legal.any(axis=1)
    rv, v = mc.to_np(got.root_visits), mc.to_np(got.visits)
    assert (rv == I * K).all()
    assert np.array_equal(v.sum(axis=1)[live], rv[live]) and not v[~live].any()
    assert not v[~legal].any()


def test_uct_5x5_reaches_terminal_nodes():
    """I well past the root's 26 actions: the walk goes deep enough to find nodes whose game has ended (a pass after a
    pass) and evaluates them in place; whole tree compared."""
    from gymgo_amd import gogame
    N, K, I = 5, 4, 90
    roots = np.concatenate([mc.crafted_roots(N)[1:2], mc.make_roots(N, 4, 31, max_ply=20, step=6)[1:3]])
    want = mc.expected_uct(roots, I, K, c=0.7, base_seed=13)
    terminal = sum(1 for t in want['trees'] for x in range(len(t.boards)) if x and t.legal[x].size == 0)
    assert terminal > 0
    got = gogame.batch_uct(roots, I, K, c=0.7, seed=13, slots=64, tree=True)   # NumPy in, NumPy out
    assert isinstance(got.visits, np.ndarray) and got.visits.dtype == np.int32 and got.plies_sum.dtype == np.int64
    assert got.legal.dtype == np.bool_ and got.nodes.dtype == np.int32 and got.tree.parent.dtype == np.int32
    _check(got, want, tree=True)
    _invariants(got, roots, I, K)


@pytest.mark.parametrize('N', [7, 9])
def test_uct_mid_game_and_crafted_roots(N):
    import torch
    from gymgo_amd import gogame
    K, I = 4, 3 * N * N // 2
    roots = np.concatenate([mc.make_roots(N, 4, 50 + N, max_ply=N * N, step=N)[1:3], mc.crafted_roots(N)])
    want = mc.expected_uct(roots, I, K, base_seed=N)
    r = mc.to_dev(roots)
    before = r.clone()
    got = gogame.batch_uct(r, I, K, seed=N, tree=True)
    assert got.legal.dtype == torch.bool and got.visits.dtype == torch.int32 and got.unfinished.dtype == torch.int64
    _check(got, want, tree=True)
    assert bool((r == before).all())
    _invariants(got, roots, I, K)
    ko = roots.shape[0] - 2
    assert not mc.to_np(got.legal)[ko, mc.KO_POINT[0] * N + mc.KO_POINT[1]]
    assert mc.to_np(got.nodes)[-1] == 1 and not mc.to_np(got.legal)[-1].any()     # the ended root: no child, K playouts per iteration
    assert np.array_equal(mc.to_np(gogame.uct_actions(r, I, K, seed=N)), mc.most_visited(want))


def test_uct_19x19_komi_and_first_root():
    from gymgo_amd import gogame
    K, I, f0 = 2, 5, 3
    roots = np.concatenate([mc.make_roots(19, 3, 7, max_ply=120, step=60)[1:3], mc.crafted_roots(19)[2:3]])
    want = mc.expected_uct(roots, I, K, komi=7.5, base_seed=17, first_root=f0)
    got = gogame.batch_uct(mc.to_dev(roots), I, K, komi=7.5, seed=17, first_root=f0, slots=512, tree=True)
    _check(got, want, tree=True)
    one = gogame.uct(mc.to_dev(roots[1]), I, K, komi=7.5, seed=17, first_root=f0 + 1, tree=True)
    for k in mc.ROOT_KEYS:
        assert np.array_equal(mc.to_np(getattr(one, k)), want[k][1]), k
    for k in mc.TREE_KEYS:
        assert np.array_equal(mc.to_np(getattr(one.tree, k)), want['tree'][k][1]), k


BIG = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
import torch
from gymgo_amd import gogame, _lib
import mc_expect as mc
assert int(_lib.lib().gg_device_cus()) == 4
# 19x19 leaves: R K = 1 536 jobs on 1 024 slots (k_rollout5, refills), 2 048 (clamped to the 1 536 jobs: k_rollout5, no
# refill), 256 (k_rollout4) and 48 (k_rollout_lat)
roots = np.concatenate([mc.make_roots(19, 4, 77, max_ply=200, step=90)[1:3], mc.crafted_roots(19)[1:2]])
I, K = 3, 512
want = mc.expected_uct(roots, I, K, komi=7.5, base_seed=19)
for S in (1024, 2048, 256, 48):
    got = gogame.batch_uct(torch.from_numpy(roots).cuda(), I, K, komi=7.5, seed=19, slots=S, tree=True)
    for k in mc.ROOT_KEYS:
        assert np.array_equal(getattr(got, k).cpu().numpy(), want[k]), (S, k)
    for k in mc.TREE_KEYS:
        assert np.array_equal(getattr(got.tree, k).cpu().numpy(), want['tree'][k]), (S, 'tree', k)
print('UCT OK')
'''


def test_uct_on_all_three_rollout_families():
    """A four-CU view of the device (GYMGO_AMD_CUS=4): 1 024 / 2 048 slots run the leaf playouts on the thirty-two-board
    kernel (k_rollout5), 256 on the sixteen-board kernel (k_rollout4), 48 on the one-row-per-lane kernel (k_rollout_lat)."""
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    script = BIG % {'root': os.path.dirname(HERE), 'here': HERE}
    p = subprocess.run([sys.executable, '-c', script], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'UCT OK' in p.stdout


def test_uct_invariant_under_slots_chunks_and_shards():
    import torch
    from gymgo_amd import gogame
    N, R, K, I = 9, 8, 4, 40
    roots = mc.make_roots(N, R, 62, max_ply=80, step=10)
    want = mc.expected_uct(roots, I, K, c=1.1, max_plies=640, komi=0.5, base_seed=5)
    r = mc.to_dev(roots)
    for S, cp in ((48, 32), (256, 16), (1024, 64), (7, 32)):
        _check(gogame.batch_uct(r, I, K, c=1.1, max_plies=640, komi=0.5, seed=5, slots=S, chunk_plies=cp, tree=True), want,
               tree=True, tag=(S, cp))
    a = gogame.batch_uct(r[:3], I, K, c=1.1, max_plies=640, komi=0.5, seed=5, slots=100)
    b = gogame.batch_uct(r[3:], I, K, c=1.1, max_plies=640, komi=0.5, seed=5, first_root=3, slots=100)
    _check(gogame.Uct(*[torch.cat([x, y]) for x, y in zip(a[:-1], b[:-1])], tree=None), want, tag='shards')
    # a cap of 64 plies: cut-off playouts are scored as they stand and counted
    cut = mc.expected_uct(roots, 6, K, c=1.1, max_plies=64, komi=0.5, base_seed=5)
    assert cut['unfinished'].sum() > 0
    _check(gogame.batch_uct(r, 6, K, c=1.1, max_plies=64, komi=0.5, seed=5, chunk_plies=16), cut, tag='cut')
    # c = 0: pure exploitation, still bit-exact
    greedy = mc.expected_uct(roots[:3], 30, K, c=0.0, max_plies=640, base_seed=5)
    _check(gogame.batch_uct(r[:3], 30, K, c=0.0, max_plies=640, seed=5), greedy, tag='c0')


def test_uct_empty_ended_and_argument_errors():
    import torch
    from gymgo_amd import gogame
    N = 9
    got = gogame.batch_uct(torch.zeros((0, 6, N, N), dtype=torch.uint8, device='cuda'), 3, 4, tree=True)
    assert got.legal.shape == (0, N * N + 1) and got.nodes.shape == (0,) and got.tree.parent.shape == (0, 4)
    ended = np.repeat(mc.crafted_roots(N)[3:], 3, axis=0)
    got = gogame.batch_uct(mc.to_dev(ended), 4, 4, tree=True)
    assert not bool(got.legal.any()) and got.nodes.tolist() == [1, 1, 1] and got.root_visits.tolist() == [16, 16, 16]
    assert got.plies_sum.tolist() == [0, 0, 0] and not bool(got.visits.any())
    assert gogame.uct_actions(mc.to_dev(ended), 4, 4).tolist() == [-1, -1, -1]
    roots = mc.to_dev(mc.make_roots(N, 2, 3, max_ply=20, step=10))
    for bad in (dict(iterations=0), dict(c=-1.0), dict(c=math.inf), dict(c=math.nan), dict(iterations=2 ** 16, playouts=2 ** 15),
                dict(playouts=0), dict(max_plies=48)):
        kw = dict(iterations=2, playouts=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            gogame.batch_uct(roots, **kw)


def test_uct_actions():
    from gymgo_amd import gogame
    N, K, I = 7, 8, 60
    roots = np.concatenate([mc.make_roots(N, 6, 3, max_ply=40, step=6)[:-1], mc.crafted_roots(N)])
    res = gogame.batch_uct(roots, I, K, komi=0.5, seed=4)
    act = gogame.uct_actions(roots, I, K, komi=0.5, seed=4)   # NumPy in, NumPy out
    assert isinstance(act, np.ndarray) and act.dtype == np.int64
    assert np.array_equal(act, mc.most_visited(res))
    assert act[-1] == -1 and (act[:-1] >= 0).all()
    # the crafted race: black to move, one move captures the top group and decides it; the search finds it
    cap = mc.capture_root()
    assert gogame.uct_actions(cap[None], 200, 64, seed=3).tolist() == [mc.CAPTURE_MOVE]
