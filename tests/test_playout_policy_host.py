"""CPU: the `no_eye_fill` playout policy without a device - the rule (mc_policy_expect.eyes) on crafted positions point by point,
the properties of the ply-by-ply expectation (mc_policy_expect.policy_rollout) that the GPU tests compare against, and the
argument checks of the Python API and the C entry points."""
import numpy as np
import pytest

import mc_expect as mc
import mc_policy_expect as mp
from oracle import c_oracle


@pytest.fixture(scope='module')
def built(native_built):
    from gymgo_amd import _lib
    return _lib


def test_eyes_on_crafted_positions_point_by_point():
    boards, want = mp.crafted_eye_boards()
    assert len(boards) == 2 * len(mp.CRAFTED)
    for i, (b, w) in enumerate(zip(boards, want)):
        got = mp.eyes(b[None])[0]
        N = b.shape[-1]
        for y in range(N):
            for x in range(N):
                assert bool(got[y, x]) == bool(w[y, x]), (mp.CRAFTED[i % len(mp.CRAFTED)][0], i >= len(mp.CRAFTED), y, x)
    # the mover's eyes only: the same stones with the other colour to move have none
    for _, rows, pts in mp.CRAFTED:
        if pts:
            assert not mp.eyes(mp.board(rows, white_to_move=True)[None]).any()
    # a game that has ended has no eyes
    b = boards[0].copy()
    b[5] = 1
    assert not mp.eyes(b[None]).any()


def test_policy_rollout_properties_9x9():
    N, B = 9, 64
    st = np.zeros((B, 6, N, N), np.uint8)
    rng0 = c_oracle.rng_seed(1, B)
    trace = []
    fin, rng1, last, steps = mp.policy_rollout(st, rng0, 8 * N * N, auto_reset=False, trace=trace)
    passes = 0
    for live, before, n, act in trace:
        e = mp.eyes(before).reshape(len(live), -1)
        pt = act < N * N
        rows = np.flatnonzero(pt)
        assert not e[rows, act[rows]].any()                                  # no played point was an eye of its mover
        assert not before[rows, 3].reshape(len(rows), N * N)[np.arange(len(rows)), act[rows]].any()   # ... nor an invalid point
        assert np.array_equal(~pt, n == 0)                                   # a pass happens only with n = 0
        passes += int((~pt).sum())
    assert passes >= 2 * B
    assert np.array_equal(mc.plies_from_rng(rng0, rng1), steps)              # the generator advanced by plies * c
    assert (fin[:, 5, 0, 0] == 1).all() and steps.max() < 8 * N * N          # every game ended (by two passes)
    assert (last == N * N).all()
    b, w = c_oracle.batch_areas(fin)
    assert np.array_equal(np.asarray(b) + np.asarray(w), np.full(B, N * N))  # no point is neutral
    # shorter than the uniform playouts of the same generators
    _, rng_u, _ = c_oracle.batch_rollout(st, rng0.copy(), 8 * N * N, auto_reset=False)
    assert steps.mean() < mc.plies_from_rng(rng0, rng_u).mean()


def test_policy_rollout_auto_reset_and_frozen_boards():
    N = 5
    roots = np.concatenate([mc.crafted_roots(N), mp.forced_pass_roots(N)])
    rng0 = c_oracle.rng_seed(3, len(roots))
    fin, rng1, last, steps = mp.policy_rollout(roots, rng0, 40, auto_reset=False)
    assert steps[3] == 0 and last[3] == -1 and rng1[3] == rng0[3] and np.array_equal(fin[3], roots[3])   # the finished game
    assert steps[4] == 2 and last[4] == N * N                                                           # pass, pass
    fin2, rng2, last2, steps2 = mp.policy_rollout(roots, rng0, 40, auto_reset=True)
    assert (steps2 == 40).all() and np.array_equal(mc.plies_from_rng(rng0, rng2), steps2)


def test_expected_policy_results_are_consistent():
    N, R, K = 5, 6, 4
    roots = mc.make_roots(N, R, 9, max_ply=24, step=4)
    full = mp.expected_playouts_policy(roots, K, 8 * N * N, with_ownership=True)
    assert np.array_equal(full['black_wins'] + full['white_wins'] + full['draws'], np.full(R, K))
    assert full['plies_sum'][-1] == 0
    a = mp.expected_playouts_policy(roots[:2], K, 8 * N * N, first_root=0)
    b = mp.expected_playouts_policy(roots[2:], K, 8 * N * N, first_root=2)
    for k in ('black_wins', 'margin_sum', 'plies_sum'):
        assert np.array_equal(np.concatenate([a[k], b[k]]), full[k])
    mv = mp.expected_move_playouts_policy(roots[:2], 2, 8 * N * N)
    assert np.array_equal(mv['legal'], mc.legal_mask(roots[:2]))
    u = mp.expected_uct_policy(roots[:2], 3, 2)
    assert (u['root_visits'] == 6).all()


def test_python_api_rejects_unknown_policy_before_a_device_is_touched():
    from gymgo_amd import gogame
    st = np.zeros((2, 6, 5, 5), np.uint8)
    for bad in ('eye', 'NO_EYE_FILL', 1, None):
        with pytest.raises(ValueError):
            gogame.batch_playouts(st, 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.playouts(st[0], 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.batch_move_playouts(st, 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.move_playouts(st[0], 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.flat_mc_actions(st, 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.batch_uct(st, 2, 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.uct(st[0], 2, 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.uct_actions(st, 2, 2, policy=bad)
        with pytest.raises(ValueError):
            gogame.batch_rollout_tracked(None, None, 1, policy=bad)
    assert gogame.POLICIES == {'uniform': 0, 'no_eye_fill': 1}


def test_policy_entry_points_check_arguments_without_device(built):
    L = built.lib()
    p = 1

    def rollout(policy=1, plies=1, B=4, N=9, ptr=1):
        q = ptr or None
        return L.gg_batch_rollout_tracked_policy(q, q, None, None, B, N, plies, 0, policy, None)

    def po(policy=1, chunks=1, N=9, K=2, ptr=1):
        q = ptr or None
        return L.gg_playouts_advance_policy(q, 4, N, K, 0, 7, 64, 32, 0.0, chunks, policy, q, q, q, q, 8, q, q, q, None, None)

    def mvp(policy=1, chunks=1, N=9, K=2, ptr=1):
        q = ptr or None
        return L.gg_move_playouts_advance_policy(q, 4, N, q, 3, K, 0, 7, 64, 32, 0.0, chunks, policy, q, q, q, q, 8, q, q, q, None)

    for call in (rollout, po, mvp):
        assert call(policy=2) == -3 and call(policy=-1) == -3
        assert call(N=1) == -1 and call(N=20) == -1
    assert rollout(plies=-1) == -3 and rollout(B=-1) == -1 and rollout(B=0) == 0
    assert rollout(ptr=0) == -2 and rollout(policy=0, ptr=0) == -2
    for call in (po, mvp):
        assert call(K=0) == -3 and call(chunks=-1) == -3
        assert call(ptr=0) == -2 and call(policy=0, ptr=0) == -2
    assert L.gg_batch_eye_mask(None, None, 4, 9, None) == -2
    assert L.gg_batch_eye_mask(p, None, 4, 20, None) == -1
    assert L.gg_batch_eye_mask(None, None, 0, 9, None) == 0


def test_eye_mask_has_no_cpu_fallback(built):
    import torch
    from gymgo_amd import gogame
    if torch.cuda.is_available():
        pytest.skip('device present')
    with pytest.raises(built.GymGoNativeError):
        gogame.batch_eye_mask(np.zeros((2, 6, 9, 9), np.uint8))
    with pytest.raises(built.GymGoNativeError):
        gogame.eye_mask(np.zeros((6, 9, 9), np.uint8))


def test_integration_document_names_the_policy_entry_points():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'INTEGRATION.md')).read()
    for name in ('gg_batch_eye_mask', 'gg_batch_rollout_tracked_policy', 'gg_playouts_advance_policy',
                 'gg_move_playouts_advance_policy', 'GG_POLICY_NO_EYE_FILL'):
        assert name in text, name
