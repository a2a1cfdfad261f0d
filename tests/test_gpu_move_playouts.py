"""-m gpu: flat Monte Carlo (gogame.batch_move_playouts: gg_move_playouts_plan / _begin / _advance, the harvest kernel of
gg_po.h with the first move played on refill) - every (root, action) output equal to the C restatement's replay of every
playout (tests/mc_expect.py) and to batch_playouts on the padded children, on all three rollout families, with
and without refills, and invariant under the slot count, the chunk length and sharding by root; flat_mc_actions."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mc_expect as mc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ('legal',) + mc.KEYS


def _check(got, want, tag=''):
    mc.check(got, want, FIELDS, tag)


@pytest.mark.parametrize('N', [7, 9])
def test_move_playouts_against_the_restatement(N):
    """Mid-game roots and the crafted ones (empty board, pass child that ends the game, active ko point, finished game),
    on 48 slots: every slot is refilled many times."""
    from gymgo_amd import gogame
    roots = np.concatenate([mc.make_roots(N, 10, 20 + N, max_ply=N * N, step=N), mc.crafted_roots(N)])
    want = mc.expected_move_playouts(roots, 4, -(-8 * N * N // 32) * 32, komi=0.0, base_seed=N)
    got = gogame.batch_move_playouts(roots, 4, komi=0.0, seed=N, slots=48)   # NumPy in, NumPy out
    assert isinstance(got.legal, np.ndarray) and got.legal.dtype == np.bool_
    _check(got, want)
    i = roots.shape[0] - 3   # the pass root: its pass child is terminal, K finished playouts of 0 plies
    assert got.legal[i, N * N] and got.plies_sum[i, N * N] == 0 and got.unfinished[i, N * N] == 0
    assert not got.legal[i + 1, mc.KO_POINT[0] * N + mc.KO_POINT[1]] and not got.legal[-1].any()


def test_move_playouts_19x19_against_the_restatement():
    from gymgo_amd import gogame
    roots = np.concatenate([mc.make_roots(19, 3, 5, max_ply=120, step=60)[:2], mc.crafted_roots(19)])
    want = mc.expected_move_playouts(roots, 2, 2912, komi=7.5, base_seed=11, first_root=3)
    r = mc.to_dev(roots)
    before = r.clone()
    got = gogame.batch_move_playouts(r, 2, max_plies=2912, komi=7.5, seed=11, first_root=3, slots=512)
    _check(got, want)
    assert bool((r == before).all())


@pytest.mark.parametrize('N,R,K', [(19, 6, 4), (13, 10, 4)])
def test_move_playouts_equal_batch_playouts_on_the_children(N, R, K):
    """Every legal row equals batch_playouts of the root's padded children with first_root = (first_root + r) A (the whole
    batch at once: child a of root r is padded slot r A + a)."""
    import torch
    from gymgo_amd import gogame
    roots = mc.to_dev(mc.make_roots(N, R + 1, 40 + N, max_ply=N * N // 2, step=N * N // (2 * R))[:R])
    A, f0 = N * N + 1, 7
    got = gogame.batch_move_playouts(roots, K, komi=7.5, seed=2, first_root=f0)
    kids = gogame.batch_children(roots).reshape(R * A, 6, N, N)
    ref = gogame.batch_playouts(kids, K, komi=7.5, seed=2, first_root=f0 * A)
    legal = got.legal.reshape(-1)
    assert bool((got.legal == (1 - gogame.batch_valid_moves(roots) == 0)).all())
    assert int(legal.sum()) < R * A
    for k in mc.KEYS:
        g = getattr(got, k).reshape(-1)
        assert bool((g[legal] == getattr(ref, k)[legal]).all()), k
        assert not bool(g[~legal].any()), k


BIG = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
import torch
from gymgo_amd import gogame, _lib
import mc_expect as mc
assert int(_lib.lib().gg_device_cus()) == 4
# 19x19: 1 024 slots (k_rollout5) with refills, 2 048 (k_rollout5) without, 256 (k_rollout4) and 48 (k_rollout_lat) with
roots = np.concatenate([mc.make_roots(19, 4, 77, max_ply=200, step=90)[1:3], mc.crafted_roots(19)[1:2]])
want = mc.expected_move_playouts(roots, 2, 2912, komi=7.5, base_seed=19)
J = int(want['legal'].sum()) * 2
assert 1024 < J <= 2048, J
for S in (1024, 2048, 256, 48):
    got = gogame.batch_move_playouts(torch.from_numpy(roots).cuda(), 2, komi=7.5, seed=19, slots=S)
    for k in ('legal',) + mc.KEYS:
        assert np.array_equal(getattr(got, k).cpu().numpy(), want[k]), (S, k)
roots9 = mc.make_roots(9, 24, 78, max_ply=60, step=3)
want9 = mc.expected_move_playouts(roots9, 8, 672, komi=7.5, base_seed=9)
got9 = gogame.batch_move_playouts(torch.from_numpy(roots9).cuda(), 8, komi=7.5, seed=9, slots=1024)
for k in ('legal',) + mc.KEYS:
    assert np.array_equal(getattr(got9, k).cpu().numpy(), want9[k]), (9, k)
print('MP OK')
'''


def test_move_playouts_on_all_three_rollout_families():
    """A four-CU view of the device (GYMGO_AMD_CUS=4): 1 024 / 2 048 slots run the chunks on the thirty-two-board kernel
    (k_rollout5), 256 on the sixteen-board kernel (k_rollout4), 48 on the one-row-per-lane kernel (k_rollout_lat)."""
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    script = BIG % {'root': os.path.dirname(HERE), 'here': HERE}
    p = subprocess.run([sys.executable, '-c', script], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'MP OK' in p.stdout


def test_move_playouts_invariant_under_slots_chunks_and_shards():
    import torch
    from gymgo_amd import gogame
    N, R, K = 9, 20, 4
    roots = mc.make_roots(N, R, 61, max_ply=80, step=4)
    want = mc.expected_move_playouts(roots, K, 704, komi=0.5, base_seed=77)
    r = mc.to_dev(roots)
    for S, cp in ((48, 32), (256, 16), (1024, 64), (256, 32)):
        _check(gogame.batch_move_playouts(r, K, max_plies=704, komi=0.5, seed=77, slots=S, chunk_plies=cp), want, (S, cp))
    a = gogame.batch_move_playouts(r[:7], K, max_plies=704, komi=0.5, seed=77, slots=200)
    b = gogame.batch_move_playouts(r[7:], K, max_plies=704, komi=0.5, seed=77, first_root=7, slots=200)
    _check(gogame.MovePlayouts(*[torch.cat([x, y]) for x, y in zip(a, b)]), want, 'shards')
    one = gogame.move_playouts(r[5], K, max_plies=704, komi=0.5, seed=77, first_root=5)
    for k in FIELDS:
        assert np.array_equal(mc.to_np(getattr(one, k)), want[k][5]), k
    # a cap of 64 plies: most playouts are cut off, scored as they stand and counted as unfinished
    cut = mc.expected_move_playouts(roots, K, 64, komi=0.5, base_seed=77)
    assert cut['unfinished'].sum() > want['legal'].sum() * K // 2
    _check(gogame.batch_move_playouts(r, K, max_plies=64, komi=0.5, seed=77, slots=100, chunk_plies=16), cut, 'cut')
    # komi 0 vs 7.5: the same playouts, wins move into draws and white's column as the replay says
    for komi in (0.0, 7.5):
        w = mc.expected_move_playouts(roots, K, 704, komi=komi, base_seed=77)
        got = gogame.batch_move_playouts(r, K, max_plies=704, komi=komi, seed=77)
        _check(got, w, komi)
        assert np.array_equal(mc.to_np(got.margin_sum), want['margin_sum'])
    assert w['white_wins'].sum() > mc.expected_move_playouts(roots, K, 704, komi=0.0, base_seed=77)['white_wins'].sum()


def test_move_playouts_empty_and_ended_batches():
    import torch
    from gymgo_amd import gogame
    N = 9
    got = gogame.batch_move_playouts(torch.zeros((0, 6, N, N), dtype=torch.uint8, device='cuda'), 4)
    assert got.legal.shape == (0, N * N + 1) and got.plies_sum.shape == (0, N * N + 1)
    ended = np.repeat(mc.crafted_roots(N)[3:], 3, axis=0)
    got = gogame.batch_move_playouts(mc.to_dev(ended), 4)
    assert got.legal.shape == (3, N * N + 1) and not bool(got.legal.any())
    for k in mc.KEYS:
        assert not bool(getattr(got, k).any()), k
    assert gogame.flat_mc_actions(mc.to_dev(ended), 4).tolist() == [-1, -1, -1]


def test_flat_mc_actions():
    from gymgo_amd import gogame
    N = 7
    roots = np.concatenate([mc.make_roots(N, 12, 3, max_ply=40, step=3)[:-1], mc.crafted_roots(N)])   # (make_roots' last: ended)
    res = gogame.batch_move_playouts(mc.to_dev(roots), 8, komi=0.5, seed=4)
    act = gogame.flat_mc_actions(mc.to_dev(roots), 8, komi=0.5, seed=4)
    res_np = gogame.MovePlayouts(*[mc.to_np(t) for t in res])
    assert np.array_equal(mc.to_np(act), mc.flat_mc_choice(roots, res_np))
    assert mc.to_np(act)[-1] == -1 and (mc.to_np(act)[:-1] >= 0).all()
    # the crafted race: black to move, one move captures the top group and decides it
    cap = mc.capture_root()
    pick = gogame.flat_mc_actions(cap[None], 256, seed=3)   # NumPy in, NumPy out
    assert isinstance(pick, np.ndarray) and pick.tolist() == [mc.CAPTURE_MOVE]
