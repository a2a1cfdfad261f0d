"""-m gpu: the plane kernels that speak about a move's child - k_moves (gg_moves.h), k_hash / k_move_hashes (gg_hash.h) - and
k_features / k_group_liberties (gg_feat.h) on THOUSANDS of game positions per board size, 2 to 19, every byte equal to what
tests/plane_scale.py reads off the children the pinned C oracle builds: the stones a move captures, the liberties and the
size of its chain, the child's hash, the capturing and the ko point.  Positions: oracle rollouts at eight depths (2 048 boards
up to 9x9, 1 024 up to 13x13, 512 above) and the children that carry a ko point; and the same boards with plane 3 holding only
the stones, where suicides and ko points are candidates.  One launch per entry point.
The repeat mask: every live (game, ply) board of 256 oracle games with its game's positions as its history, expected by
comparing positions stone by stone - a repeat the kernel reports and that comparison does not is a hash collision or a bug,
and fails.  tests/test_plane_scale_host.py holds what this file relies on.  (The life and ladder planes have no counterpart in
the oracle: tests/test_gpu_plane_trips.py takes them past one grid against their definitional modules.)"""
import numpy as np
import pytest

import hash_expect as he
import mc_expect as mc
import plane_cases as pc
import plane_scale as ps
import test_gpu_features as tgf

pytestmark = pytest.mark.gpu

same = tgf.same


@pytest.mark.parametrize('N', ps.SIZES)
def test_game_positions_against_the_oracles_children(N):
    import torch
    from gymgo_amd import gogame
    c = ps.positions(N)
    r = c.ref
    B = len(c.states)
    st = mc.to_dev(c.states.copy())             # (the cached arrays are read-only)
    tracked = gogame.batch_track(st)
    same(gogame.batch_group_liberties(st), r.libs, (N, 'group liberties'))
    same(gogame.batch_features(st, dtype=torch.uint8), r.features, (N, 'features'))
    got = gogame.batch_features(st, dtype=torch.float16)
    assert got.dtype == torch.float16
    same(got.to(torch.uint8), r.features, (N, 'features, float16'))
    same(gogame.batch_features_tracked(tracked, dtype=torch.uint8), r.features, (N, 'features, tracked'))
    same(gogame.batch_move_counts(st), r.counts, (N, 'move counts'))
    same(gogame.batch_move_planes(st, dtype=torch.uint8), r.planes, (N, 'move planes'))
    same(gogame.batch_move_planes_tracked(tracked, dtype=torch.uint8), r.planes, (N, 'move planes, tracked'))
    same(gogame.batch_hash(st), r.hashes, (N, 'hash'))
    same(gogame.batch_hash_tracked(tracked), r.hashes, (N, 'hash, tracked'))
    same(gogame.batch_move_hashes(st), r.moves, (N, 'move hashes'))
    same(gogame.batch_move_hashes_tracked(tracked), r.moves, (N, 'move hashes, tracked'))
    orient = (np.arange(B) & 7).astype(np.int32)
    o = torch.from_numpy(orient).cuda()
    same(gogame.batch_features(st, dtype=torch.uint8, orient=o), pc.turned(r.features, orient), (N, 'features, oriented'))
    same(gogame.batch_move_planes(st, dtype=torch.uint8, orient=o), pc.turned(r.planes, orient), (N, 'move planes, oriented'))


@pytest.mark.parametrize('N', ps.SIZES)
def test_plane_3_holding_only_the_stones(N):
    """Suicides (rule 4: all three counts 0, the hash that of the child with the played chain on the board) and the ko point as
    candidates.  Byte planes only: a tracked board made from these has true invalid rows."""
    import torch
    from gymgo_amd import gogame
    c = ps.positions(N)
    r = c.ref_open
    st = mc.to_dev(c.open.copy())
    same(gogame.batch_features(st, dtype=torch.uint8), r.features, (N, 'features'))
    same(gogame.batch_move_counts(st), r.counts, (N, 'move counts'))
    same(gogame.batch_move_planes(st, dtype=torch.uint8), r.planes, (N, 'move planes'))
    same(gogame.batch_hash(st), r.hashes, (N, 'hash'))
    same(gogame.batch_move_hashes(st), r.moves, (N, 'move hashes'))


@pytest.mark.parametrize('N', ps.GAME_SIZES)
def test_repeat_masks_of_whole_games_stone_by_stone(N):
    import torch
    from gymgo_amd import gogame
    import test_gpu_hash as tgh
    g = ps.games(N)
    M, P = len(g.states), N * N
    st = mc.to_dev(g.states.copy())
    tracked = gogame.batch_track(st)
    history = tgh.history_of(g.history.copy(), g.count.copy())      # (the cached arrays are read-only)
    got = gogame.batch_superko_moves(st, history)
    assert got.dtype == torch.uint8
    same(got, g.mask, (N, 'bytes'))
    same(gogame.batch_superko_moves_tracked(tracked, history), g.mask, (N, 'tracked'))
    # in place on a clone: plane 3 becomes the old plane ORed with the mask, nothing else changes
    st2 = st.clone()
    assert gogame.batch_forbid_repeats(st2, history) is st2
    after = mc.to_np(st2)
    assert np.array_equal(after[:, 3], g.states[:, 3] | g.mask[:, :P].reshape(M, N, N)), N
    assert np.array_equal(np.delete(after, 3, axis=1), np.delete(g.states, 3, axis=1)), N
    t2 = tracked.clone()
    assert gogame.batch_forbid_repeats_tracked(t2, history) is t2
    t0, t1 = mc.to_np(tracked), mc.to_np(t2)
    assert np.array_equal(t1[:, 2 * N:3 * N], t0[:, 2 * N:3 * N] | he.rows_of(g.mask, N)), N
    assert np.array_equal(np.delete(t1, np.s_[2 * N:3 * N], axis=1), np.delete(t0, np.s_[2 * N:3 * N], axis=1)), N
