"""CPU: flat Monte Carlo (gg_move_playouts_plan / _begin / _advance, gogame.batch_move_playouts) without a device - argument
checks of the C-ABI, no CPU fallback in the Python API, and the expectation helpers the GPU tests build on
(tests/mc_expect.py) against the C restatement."""
import numpy as np
import pytest

import mc_expect as mc
from oracle import c_oracle


@pytest.fixture(scope='module')
def built(native_built):
    from gymgo_amd import _lib
    return _lib


def _plan(L, R=4, N=9, ptr=1):
    p = ptr or None
    return L.gg_move_playouts_plan(p, R, N, p, p, None)


def _begin(L, R=4, N=9, T=3, K=2, first_root=0, max_plies=64, chunk=32, S=8, ptr=1):
    p = ptr or None
    return L.gg_move_playouts_begin(p, R, N, p, T, K, first_root, 7, max_plies, chunk, p, p, p, p, S, p, p, p, None)


def _advance(L, R=4, N=9, T=3, K=2, first_root=0, max_plies=64, chunk=32, chunks=1, S=8, ptr=1):
    p = ptr or None
    return L.gg_move_playouts_advance(p, R, N, p, T, K, first_root, 7, max_plies, chunk, 0.0, chunks, p, p, p, p, S, p, p, p,
                                      None)


def test_move_playout_entry_points_check_arguments_before_device_work(built):
    L = built.lib()
    for call in (_plan, _begin, _advance):
        assert call(L, N=1) == -1 and call(L, N=20) == -1
        assert call(L, R=-1) == -1
        assert call(L, R=(2 ** 31 - 1) // 362 + 1, N=19) == -1     # R (N^2 + 1) does not fit an int32
        assert call(L, ptr=0) == -2
    for call in (_begin, _advance):
        assert call(L, S=0) == -1
        assert call(L, T=-1) == -1 and call(L, R=4, N=9, T=4 * 82 + 1) == -1
        assert call(L, K=0) == -3
        assert call(L, chunk=0) == -3
        assert call(L, max_plies=48, chunk=32) == -3
        assert call(L, max_plies=0) == -3
        assert call(L, first_root=-1) == -3
        assert call(L, first_root=2 ** 62 // 82, K=1) == -1          # global job ids beyond an int64
    assert _advance(L, chunks=-1) == -3
    # (valid arguments with NULL buffers are still a NULL-pointer error, not a launch; nothing to do is not an error)
    assert _advance(L, chunks=0, ptr=0) == -2


def test_batch_move_playouts_has_no_cpu_fallback(built):
    import torch
    from gymgo_amd import gogame
    if torch.cuda.is_available():
        pytest.skip('device present')
    with pytest.raises(built.GymGoNativeError):
        gogame.batch_move_playouts(np.zeros((2, 6, 9, 9), np.uint8), 4)
    with pytest.raises(built.GymGoNativeError):
        gogame.move_playouts(np.zeros((6, 9, 9), np.uint8), 4)
    with pytest.raises(built.GymGoNativeError):
        gogame.batch_move_playouts(torch.zeros((2, 6, 9, 9), dtype=torch.uint8), 4)
    with pytest.raises(built.GymGoNativeError):
        gogame.flat_mc_actions(np.zeros((2, 6, 9, 9), np.uint8), 4)


def test_job_seed_restatement_matches_the_c_generator():
    L = c_oracle.lib()
    ids = np.concatenate([np.arange(0, 300), np.array([12345, 2 ** 31 - 1, 2 ** 31, 2 ** 40 + 7, 3 * 2 ** 50 + 11, 2 ** 62 - 1])])
    for seed in (0, 20260927, 2 ** 64 - 1):
        want = np.array([L.gg_oracle_rng_seed(seed, int(i)) for i in ids], np.uint64)
        assert np.array_equal(mc.po_seed(seed, ids), want)
    assert np.array_equal(mc.po_seed(5, np.arange(64)), c_oracle.rng_seed(5, 64))


@pytest.mark.parametrize('N', [5, 7, 9, 19])
def test_legal_mask_is_valid_moves_with_ended_roots_zeroed(N):
    roots = np.concatenate([mc.make_roots(N, 12, 4, max_ply=N * N, step=N), mc.crafted_roots(N)])
    legal = mc.legal_mask(roots)
    R, A = roots.shape[0], N * N + 1
    ended = roots[:, 5, 0, 0] != 0
    assert ended[-1] and ended[-5] and ended.sum() >= 2          # make_roots' finished game and the crafted one
    assert not legal[ended].any()
    valid = 1 - np.concatenate([roots[:, 3].reshape(R, -1), np.zeros((R, 1), np.uint8)], axis=1)   # gogame.valid_moves
    assert np.array_equal(legal[~ended], valid[~ended].astype(bool))
    # the same set from the restatement's children: a padded slot is all zero exactly when the move is invalid
    kids = c_oracle.batch_children(roots)
    assert np.array_equal(legal[~ended], kids[~ended].reshape(R - ended.sum(), A, -1).any(axis=2))
    # the crafted roots: the ko point may not be retaken, the pass after a pass ends the game
    ko = mc.crafted_roots(N)[2]
    assert not mc.legal_mask(ko[None])[0, mc.KO_POINT[0] * N + mc.KO_POINT[1]]
    end_kid = c_oracle.next_state(mc.crafted_roots(N)[1], N * N)
    assert end_kid[5].all()


def test_expected_move_results_are_consistent():
    N, K = 7, 6
    roots = np.concatenate([mc.make_roots(N, 6, 2, max_ply=40, step=8)[:-1], mc.crafted_roots(N)])
    e = mc.expected_move_playouts(roots, K, 8 * N * N, komi=0.0, base_seed=3)
    legal = e['legal']
    total = e['black_wins'] + e['white_wins'] + e['draws']
    assert np.array_equal(total[legal], np.full(legal.sum(), K)) and not total[~legal].any()
    for k in mc.KEYS:
        assert not e[k][~legal].any(), k
    assert e['unfinished'].sum() == 0
    # the crafted pass root: its pass child has ended, K finished playouts of 0 plies
    i = roots.shape[0] - 3
    assert e['plies_sum'][i, N * N] == 0 and e['unfinished'][i, N * N] == 0
    assert e['plies_sum'][i, :N * N][legal[i, :N * N]].min() > 0
    # row (r, a) is batch_playouts of the child alone with first_root = (first_root + r) A + a
    r, a = np.nonzero(legal)
    for r_, a_ in list(zip(r, a))[::29]:
        kid = c_oracle.next_state(roots[r_], int(a_))
        one = mc.expected_playouts(kid[None], K, 8 * N * N, komi=0.0, base_seed=3, first_root=(5 + r_) * (N * N + 1) + a_)
        sh = mc.expected_move_playouts(roots[r_:r_ + 1], K, 8 * N * N, komi=0.0, base_seed=3, first_root=5 + r_)
        for k in mc.KEYS:
            assert one[k][0] == sh[k][0, a_], k
    # shards by first_root are the whole
    s1 = mc.expected_move_playouts(roots[:4], K, 8 * N * N, base_seed=3)
    s2 = mc.expected_move_playouts(roots[4:], K, 8 * N * N, base_seed=3, first_root=4)
    for k in ('legal',) + mc.KEYS:
        assert np.array_equal(np.concatenate([s1[k], s2[k]]), e[k]), k


def test_flat_mc_choice_restatement():
    roots = mc.crafted_roots(5)
    A = 26
    res = {'legal': mc.legal_mask(roots), 'black_wins': np.zeros((4, A), np.int32), 'white_wins': np.zeros((4, A), np.int32)}
    res['black_wins'][:, 7] = 3
    res['white_wins'][:, 9] = 3
    got = mc.flat_mc_choice(roots, res)
    # the mover's wins count: action 7 for black to move, 9 for white; the finished root has no move
    turn = roots[:, 2, 0, 0]
    assert got[3] == -1
    for i in range(3):
        assert got[i] == (9 if turn[i] else 7)
    res['black_wins'][:] = 0
    res['white_wins'][:] = 0
    assert list(mc.flat_mc_choice(roots, res)[:3]) == [int(np.flatnonzero(res['legal'][i])[0]) for i in range(3)]
