"""-m gpu: the network input planes with per-group liberty counts (gogame.batch_features / batch_features_tracked /
batch_group_liberties: k_features / k_group_liberties of gg_feat.h) - every byte equal to the definitional expectation
(tests/features_expect.py): random positions of every board-size class at three depths with a ragged last wave, B = 1 and
B = 3, crafted boards (the longest flood, a group with more than 128 liberties, the row wrap, 3 next to 4 liberties, full
boards, groups without liberties, the empty board, a ko) with either colour to move; the four dtypes; tracked input against
byte-plane input, also after plies played on the tracked boards; out=, a non-default stream, NumPy in / out, B = 0; and
PuctSearch / batch_puct / puct_selfplay with features= against the same search fed batch_features of the states."""
import functools

import numpy as np
import pytest

import features_expect as fe
import mc_expect as mc

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 5, 9, 13, 19)
B_RANDOM = 257


@functools.lru_cache(maxsize=None)
def positions(N):
    """257 positions of random play (gogame.batch_rollout, auto_reset off: some games have ended) at three depths - opening,
    middle, near the end - and what is expected of them: (device states, NumPy states, planes, counts), computed once."""
    import torch
    from gymgo_amd import gogame
    parts = []
    for i, depth in enumerate((N, N * N // 2 + 1, 3 * N * N // 2)):
        n = B_RANDOM // 3 + (1 if i < B_RANDOM % 3 else 0)
        st = gogame.batch_init_state(n, N, device='cuda')
        gogame.batch_rollout(st, gogame.rng_seed(n, 100 + N + i), depth, auto_reset=False)
        parts.append(st)
    st = torch.cat(parts).contiguous()
    s = st.cpu().numpy()
    assert s.shape == (B_RANDOM, 6, N, N)
    return st, s, fe.batch_features(s), fe.batch_group_liberties(s)


@functools.lru_cache(maxsize=None)
def crafted(N):
    s = np.concatenate([fe.crafted(N), mc.crafted_roots(N)])
    return s, fe.batch_features(s), fe.batch_group_liberties(s)


def same(got, want, tag=''):
    got = mc.to_np(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want), (tag, np.argwhere(got != want)[:8])


@pytest.mark.parametrize('N', SIZES)
def test_random_positions_planes_and_counts(N):
    import torch
    from gymgo_amd import gogame
    st, s, planes, libs = positions(N)
    ended = s[:, 5, 0, 0] != 0
    assert ended.any() and not ended.all()
    same(gogame.batch_features(st, dtype=torch.uint8), planes, N)
    same(gogame.batch_group_liberties(st), libs, N)
    for B in (1, 3):        # a lone board, a wave that is not full; slices that start at any byte
        for first in (0, 100, B_RANDOM - B):
            same(gogame.batch_features(st[first:first + B], dtype=torch.uint8), planes[first:first + B], (N, B, first))
            same(gogame.batch_group_liberties(st[first:first + B]), libs[first:first + B], (N, B, first))


@pytest.mark.parametrize('N', (9, 19))
def test_crafted_boards(N):
    import torch
    from gymgo_amd import gogame
    s, planes, libs = crafted(N)
    # what the boards are there for
    on_spiral = s[0, 0] != 0
    assert len(np.unique(libs[0][on_spiral])) == 1 and libs[0][on_spiral][0] == libs[0].max() > 2 * N   # one number on the group
    assert libs[2].max() == (N - 1) // 2 * (N - 2) + (N + 1) // 2 and (N < 19 or libs[2].max() > 128)            # the comb
    assert planes[:, 11].sum() >= 1                                                                                # a ko
    assert (planes[:, 2:10].sum(axis=1)[(s[:, 0] | s[:, 1]) != 0] == 0).any()                                      # groups without liberties
    st = mc.to_dev(s)
    same(gogame.batch_features(st, dtype=torch.uint8), planes, N)
    same(gogame.batch_group_liberties(st), libs, N)
    same(gogame.batch_features_tracked(gogame.batch_track(st), dtype=torch.uint8), planes, N)
    for i in (0, 3, len(s) - 1):      # ... and one board at a time
        same(gogame.features(st[i], dtype=torch.uint8), planes[i], (N, i))
        same(gogame.group_liberties(st[i]), libs[i], (N, i))


@pytest.mark.parametrize('N', (5, 13, 19))
def test_dtypes(N):
    import torch
    from gymgo_amd import gogame
    st, s, planes, _ = positions(N)
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        got = gogame.batch_features(st, dtype=dt)
        assert got.dtype == dt and tuple(got.shape) == planes.shape
        assert bool(((got == 0) | (got == 1)).all())
        same(got.to(torch.uint8), planes, (N, dt))
        same(gogame.batch_features_tracked(gogame.batch_track(st), dtype=dt).to(torch.uint8), planes, (N, dt, 'tracked'))
    assert gogame.batch_features(st).dtype == torch.float16          # the default


@pytest.mark.parametrize('N', SIZES)
def test_tracked_input_equals_byte_planes_also_after_plies(N):
    import torch
    from gymgo_amd import gogame
    st, s, planes, _ = positions(N)
    tracked = gogame.batch_track(st)
    same(gogame.batch_features_tracked(tracked, dtype=torch.uint8), planes, N)
    rng = gogame.rng_seed(B_RANDOM, 77 + N)
    for ply in range(5):            # the classes are carried by the one-move step; ended games stay where they are
        acts = gogame.batch_sample_actions(gogame.batch_untrack(tracked), rng)
        gogame.batch_play_moves_tracked(tracked, acts[:, None])
        if ply in (0, 4):
            now = gogame.batch_untrack(tracked)
            got = gogame.batch_features_tracked(tracked, dtype=torch.uint8)
            assert bool((got == gogame.batch_features(now, dtype=torch.uint8)).all()), (N, ply)
            same(got[::8], fe.batch_features(now[::8].cpu().numpy()), (N, ply))
    assert not bool((now == st).all())


def test_plumbing_out_stream_numpy_and_empty_batch():
    import torch
    from gymgo_amd import gogame
    N = 9
    st, s, planes, libs = positions(N)
    # out=: filled and returned
    out = torch.full((B_RANDOM, 16, N, N), 7, dtype=torch.uint8, device='cuda')
    assert gogame.batch_features(st, dtype=torch.uint8, out=out) is out
    same(out, planes)
    out = torch.full((B_RANDOM, 16, N, N), 7, dtype=torch.float32, device='cuda')
    assert gogame.batch_features_tracked(gogame.batch_track(st), dtype=torch.float32, out=out) is out
    same(out.to(torch.uint8), planes)
    with pytest.raises(ValueError):
        gogame.batch_features(st, dtype=torch.float16, out=out)                      # the wrong dtype
    with pytest.raises(ValueError):
        gogame.batch_features(st, dtype=torch.float32, out=out.transpose(2, 3))      # not contiguous
    with pytest.raises(ValueError):
        gogame.batch_features(st, dtype=torch.uint8, out=torch.zeros(B_RANDOM * 16 * N * N + 1, dtype=torch.uint8, device='cuda')[1:].view(
            B_RANDOM, 16, N, N))                                                    # not 16-byte aligned
    # a non-default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = gogame.batch_features(st, dtype=torch.uint8)
        b = gogame.batch_group_liberties(st)
    side.synchronize()
    same(a, planes)
    same(b, libs)
    # NumPy in, NumPy out
    got = gogame.batch_features(s, dtype=torch.uint8)
    assert isinstance(got, np.ndarray)
    same(got, planes)
    got = gogame.batch_features(s[:5].astype(np.float64), dtype=torch.float32)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, planes[:5].astype(np.float32))
    got = gogame.batch_group_liberties(s)
    assert isinstance(got, np.ndarray) and np.array_equal(got, libs)
    assert isinstance(gogame.features(s[3]), np.ndarray) and np.array_equal(gogame.features(s[3], dtype=torch.uint8), planes[3])
    assert np.array_equal(gogame.group_liberties(s[3]), libs[3])
    # B = 0
    empty = torch.empty((0, 6, N, N), dtype=torch.uint8, device='cuda')
    assert tuple(gogame.batch_features(empty).shape) == (0, 16, N, N) and tuple(gogame.batch_group_liberties(empty).shape) == (0, N, N)
    assert tuple(gogame.batch_features_tracked(gogame.batch_track(st)[:0]).shape) == (0, 16, N, N)


# ---------------------------------------------------------------- the search
def plane_evaluator(planes, legal):
    """Deterministic and defined ON PLANES: priors proportional to 1 + 2 * (capture plane) over the legal actions (the pass
    weighs 1), value = (own stones - opponent stones) / N^2 in float32."""
    import torch
    B, N = planes.shape[0], planes.shape[-1]
    p = planes.to(torch.float32)
    w = torch.cat([1 + 2 * p[:, 12].reshape(B, N * N), torch.ones((B, 1), dtype=torch.float32, device=p.device)], dim=1)
    w = torch.where(legal, w, torch.zeros_like(w))
    priors = w / w.sum(dim=1, keepdim=True).clamp(min=1.0)
    nn = torch.full((), float(N * N), dtype=torch.float32, device=p.device)
    values = (p[:, 0].sum(dim=(1, 2)) - p[:, 1].sum(dim=(1, 2))) / nn
    return priors, values


def state_evaluator(states, legal):
    import torch
    from gymgo_amd import gogame
    assert states.dtype == torch.uint8 and states.shape[1] == 6
    return plane_evaluator(gogame.batch_features(states, dtype=torch.float16), legal)


def seen_planes(planes, legal):
    import torch
    assert planes.dtype == torch.float16 and planes.shape[1] == 16
    return plane_evaluator(planes, legal)


def search_roots(N):
    return mc.to_dev(np.concatenate([mc.make_roots(N, 4, 40 + N, max_ply=N * N, step=N), mc.crafted_roots(N)[2:3]]))   # R = 5, a ko root


def same_tuples(a, b, tag=''):
    """Every field of two (nested) namedtuples of tensors identical, floats as bit patterns."""
    import torch
    assert type(a) is type(b)
    for k in a._fields:
        x, y = getattr(a, k), getattr(b, k)
        if x is None or y is None:
            assert x is None and y is None, (tag, k)
        elif isinstance(x, tuple):
            same_tuples(x, y, (tag, k))
        else:
            assert x.dtype == y.dtype and x.shape == y.shape, (tag, k)
            if x.dtype.is_floating_point:
                x, y = x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32), y.contiguous().view(
                    torch.int64 if y.dtype == torch.float64 else torch.int32)
            assert bool((x == y).all()), (tag, k)


@pytest.mark.parametrize('N', (5, 9))
@pytest.mark.parametrize('leaves', (None, 3))
def test_puct_with_features_equals_puct_fed_batch_features(N, leaves):
    import torch
    from gymgo_amd import gogame
    roots = search_roots(N)
    assert roots.shape[0] == 5
    a = gogame.batch_puct(roots, 12, seen_planes, komi=0.5, tree=True, leaves=leaves, features=torch.float16)
    b = gogame.batch_puct(roots, 12, state_evaluator, komi=0.5, tree=True, leaves=leaves)
    same_tuples(a, b, (N, leaves))
    assert int(a.root_visits.sum()) > 5
    # step by step: the planes are batch_features of the states the features-less twin hands out, row for row (empty slots too)
    sa = gogame.PuctSearch(roots, 12, komi=0.5, leaves=leaves, features=torch.float16)
    sb = gogame.PuctSearch(roots, 12, komi=0.5, leaves=leaves)
    empty_rows = 0
    for _ in range(12):
        planes, legal_a = sa.select()
        states, legal_b = sb.select()
        rows = 5 * (leaves or 1)
        assert tuple(planes.shape) == (rows, 16, N, N) and planes.dtype == torch.float16
        assert bool((planes == gogame.batch_features(states, dtype=torch.float16)).all())
        assert bool((legal_a == legal_b).all())
        if leaves:
            assert bool((sa.live == sb.live).all())
            empty_rows += int((~sa.live).sum())
        priors, values = plane_evaluator(planes, legal_a)
        sa.backup(priors, values)
        sb.backup(priors, values)
    assert leaves is None or empty_rows > 0
    same_tuples(sa.result(tree=True), sb.result(tree=True), (N, leaves, 'steps'))
    same_tuples(sa.result(tree=True), a, (N, leaves, 'loop'))
    assert bool((sa.root_states() == roots).all())                  # root_states() is unchanged: byte planes
    # the most-visited move
    assert bool((gogame.puct_actions(roots, 12, seen_planes, komi=0.5, leaves=leaves, features=torch.float16)
                 == gogame.puct_actions(roots, 12, state_evaluator, komi=0.5, leaves=leaves)).all())


@pytest.mark.parametrize('leaves', (None, 3))
def test_selfplay_records_are_the_same_either_way(leaves):
    import torch
    from gymgo_amd import gogame
    N = 5
    roots = search_roots(N)
    kw = dict(komi=0.5, leaves=leaves, capacity=64, sample_moves=1, seed=5, record_states=True)
    a = gogame.puct_selfplay(roots, 3, 8, seen_planes, features=torch.float16, **kw)
    b = gogame.puct_selfplay(roots, 3, 8, state_evaluator, **kw)
    same_tuples(a, b, leaves)
    assert a.states.dtype == torch.uint8 and tuple(a.states.shape) == (5, 3, 6, N, N) and int(a.lengths.sum()) > 0
    pa = gogame.puct_play(roots, 2, 8, seen_planes, komi=0.5, leaves=leaves, capacity=64, features=torch.float16)
    pb = gogame.puct_play(roots, 2, 8, state_evaluator, komi=0.5, leaves=leaves, capacity=64)
    assert bool((pa[0] == pb[0]).all()) and bool((pa[1] == pb[1]).all())
    with pytest.raises(ValueError):
        gogame.batch_puct(roots, 4, gogame.playout_evaluator(2, komi=0.5), komi=0.5, features=torch.float16)
