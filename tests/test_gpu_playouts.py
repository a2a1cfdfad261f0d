"""-m gpu: batched Monte Carlo playouts (gogame.batch_playouts: gg_playouts_begin / gg_playouts_advance, the harvest kernel of
gg_po.h around the tracked rollout) - every per-root output equal to the C restatement's replay of every playout
(tests/mc_expect.py), on all three rollout families, with and without refills, cut-offs, komi, ownership, and
invariance under the slot count, the chunk length and sharding by root."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mc_expect as mc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _check(got, want, own=False):
    mc.check(got, want, mc.KEYS + (('ownership',) if own else ()))
    if not own:
        assert got.ownership is None


@pytest.fixture(scope='module')
def roots19():
    return mc.make_roots(19, 128, 101, max_ply=200, step=8)


def test_playouts_19x19_with_and_without_refills(roots19):
    """128 mid-game roots (an empty one, a finished one) x 8 on 256 slots (each refilled ~4x) and on 1 024 (no refill); the
    roots are left as they were."""
    from gymgo_amd import gogame
    want = mc.expected_playouts(roots19, 8, 2912, komi=7.5, base_seed=5)
    r = mc.to_dev(roots19)
    before = r.clone()
    for S in (256, 1024):
        got = gogame.batch_playouts(r, 8, max_plies=2912, komi=7.5, seed=5, slots=S)
        _check(got, want)
        assert bool((r == before).all())
    assert want['plies_sum'][-1] == 0 and want['unfinished'].sum() == 0


@pytest.mark.parametrize('N', [7, 9, 13])
def test_playouts_small_boards_small_slot_counts(N):
    from gymgo_amd import gogame
    roots = mc.make_roots(N, 40, 7 + N, max_ply=3 * N * N // 2, step=N)
    want = mc.expected_playouts(roots, 6, -(-8 * N * N // 32) * 32, komi=0.0, base_seed=N, with_ownership=True)
    got = gogame.batch_playouts(roots, 6, komi=0.0, seed=N, slots=48, ownership=True)   # NumPy in, NumPy out
    assert isinstance(got.black_wins, np.ndarray)
    _check(got, want, own=True)


def test_playouts_cut_off_komi_and_ownership(roots19):
    """max_plies = 64: most playouts are cut off, scored as they stand and counted as unfinished; komi 0 (draws) and negative."""
    from gymgo_amd import gogame
    r = mc.to_dev(roots19)
    for komi, cp in ((0.0, 32), (-3.5, 16)):
        want = mc.expected_playouts(roots19, 8, 64, komi=komi, base_seed=9, with_ownership=True)
        assert want['unfinished'].sum() > 512
        got = gogame.batch_playouts(r, 8, max_plies=64, komi=komi, seed=9, slots=300, chunk_plies=cp, ownership=True)
        _check(got, want, own=True)


def test_playouts_invariant_under_slots_chunks_and_shards():
    from gymgo_amd import gogame
    import torch
    N, R, K = 9, 96, 8
    roots = mc.make_roots(N, R, 33, max_ply=100, step=4)
    want = mc.expected_playouts(roots, K, 704, komi=0.5, base_seed=77, with_ownership=True)
    r = mc.to_dev(roots)
    for S, cp in ((R * K, 32), (512, 16), (96, 64), (96, 32)):
        got = gogame.batch_playouts(r, K, max_plies=704, komi=0.5, seed=77, slots=S, chunk_plies=cp, ownership=True)
        _check(got, want, own=True)
    a = gogame.batch_playouts(r[:40], K, max_plies=704, komi=0.5, seed=77, slots=128, ownership=True)
    b = gogame.batch_playouts(r[40:], K, max_plies=704, komi=0.5, seed=77, first_root=40, slots=128, ownership=True)
    cat = gogame.Playouts(*[None if x is None else torch.cat([x, y]) for x, y in zip(a, b)])
    _check(cat, want, own=True)
    one = gogame.playouts(r[5], K, max_plies=704, komi=0.5, seed=77, first_root=5)
    assert int(one.black_wins) == want['black_wins'][5] and int(one.plies_sum) == want['plies_sum'][5]


BIG = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
import torch
from gymgo_amd import gogame, _lib
import mc_expect as mc
assert int(_lib.lib().gg_device_cus()) == 4
for N, R, K in ((19, 128, 12), (9, 160, 16), (13, 160, 12)):
    roots = mc.make_roots(N, R, 500 + N, max_ply=2 * N * N // 3, step=N)
    want = mc.expected_playouts(roots, K, -(-8 * N * N // 32) * 32, komi=7.5, base_seed=N, with_ownership=N == 19)
    # 1 024 slots: k_rollout5 (more than 128 / 159 games per CU); 19x19 on 256 slots as well: k_rollout4
    for S in ((1024, 256) if N == 19 else (1024,)):
        got = gogame.batch_playouts(torch.from_numpy(roots).cuda(), K, komi=7.5, seed=N, slots=S, ownership=N == 19)
        for k in ('black_wins', 'white_wins', 'draws', 'unfinished', 'margin_sum', 'plies_sum') + (('ownership',) if N == 19 else ()):
            assert np.array_equal(getattr(got, k).cpu().numpy(), want[k]), (N, S, k)
print('PO OK')
'''


def test_playouts_on_the_big_batch_kernel():
    """1 024 slots on a four-CU view of the device (GYMGO_AMD_CUS=4): the thirty-two-board kernel (k_rollout5) serves the
    chunks at 19x19, 9x9 and 13x13 (256 slots at 19x19: the sixteen-board kernel), while the restatement can still replay
    every playout."""
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    script = BIG % {'root': os.path.dirname(HERE), 'here': HERE}
    p = subprocess.run([sys.executable, '-c', script], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'PO OK' in p.stdout
