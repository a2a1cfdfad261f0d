"""-m gpu: the move-outcome kernels (k_moves of gg_moves.h: gogame.batch_move_planes, batch_move_planes_tracked,
batch_move_counts) at EVERY board size from 2 to 19, every byte equal to the definitional expectation
(tests/outcome_expect.py; tests/test_outcome_host.py holds what this file relies on): the 21 policy positions and the 21
clean boards of tests/plane_cases.py from byte planes and tracked boards, in the dtype N % 4 picks, the counts, all eight
orientations, sub-batches written between sentinel bytes, the hand-made boards, the argument errors, and the planes
PuctSearch(outcome=True) and selfplay_batch(outcome=True) hand out."""
import numpy as np
import pytest

import mc_expect as mc
import outcome_expect as oe
import plane_cases as pc
import test_gpu_features as tgf
import test_gpu_life as tgl
import test_gpu_plane_sizes as tps
import test_gpu_symmetry_io as tsio

pytestmark = pytest.mark.gpu

B = pc.B
SETS = ('policy', 'clean')
SENTINEL = 0xA5
same = tgf.same
mixed = tgl.mixed
dtype_of = tps.dtype_of


@pytest.mark.parametrize('N', pc.SIZES)
def test_planes_and_counts_byte_planes_and_tracked(N):
    import torch
    from gymgo_amd import gogame
    dt = dtype_of(N)
    for kind in SETS:
        c = oe.case(N, kind)
        st = mc.to_dev(c.states.copy())         # (the cached arrays are read-only)
        tracked = gogame.batch_track(st)
        same(gogame.batch_move_counts(st), c.counts, (N, kind, 'counts'))
        for name, x, fn in (('bytes', st, gogame.batch_move_planes), ('tracked', tracked, gogame.batch_move_planes_tracked)):
            got = fn(x)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (B, 12, N, N)
            same(got, c.planes, (N, kind, name))
            got = fn(x, dtype=dt)
            assert got.dtype == dt
            same(got.to(torch.uint8), c.planes, (N, kind, name, dt))
            assert bool(((got == 0) | (got == 1)).all())


@pytest.mark.parametrize('N', pc.SIZES)
def test_orientations(N):
    import torch
    from gymgo_amd import gogame
    orient = mixed(B)                                            # all eight views, with the negative and the large words
    assert set(orient & 7) == set(range(8)) and orient.min() < 0 and orient.max() > 7
    o = torch.from_numpy(orient).cuda()
    dt = dtype_of(N)
    for kind in SETS:
        c = oe.case(N, kind)
        st = mc.to_dev(c.states.copy())
        tracked = gogame.batch_track(st)
        want = pc.turned(c.planes, orient)
        same(gogame.batch_move_planes(st, orient=o), want, (N, kind, 'bytes'))
        same(gogame.batch_move_planes_tracked(tracked, dtype=dt, orient=orient).to(torch.uint8), want, (N, kind, 'tracked'))
        turned = gogame.batch_symmetry(st, o & 7)
        same(gogame.batch_move_planes(turned), want, (N, kind, 'the planes of the turned position'))
        same(gogame.batch_move_counts(turned), pc.turned(c.counts, orient), (N, kind, 'the counts of the turned position'))


@pytest.mark.parametrize('N', pc.SIZES)
def test_sub_batches_between_sentinels(N):
    """A lone board and a wave that is not full, from three places of the batch, written through out= into a slice of a
    larger buffer 1, 7 or 20 elements into it (out needs its element's alignment only): nothing before or behind the slice
    is written.  The counts of the same sub-batches (their input starts at any byte)."""
    import torch
    from gymgo_amd import gogame
    dt = dtype_of(N)
    size = torch.empty(0, dtype=dt).element_size()
    P = N * N
    for kind in SETS:
        c = oe.case(N, kind)
        st = mc.to_dev(c.states.copy())
        tracked = gogame.batch_track(st)
        for nb in (1, 3):
            for k, first in enumerate((0, 7, B - nb)):
                lead, sl, n = (1, 7, 20)[k], slice(first, first + nb), nb * 12 * P
                tag = (N, kind, dt, nb, first)
                raw = torch.full(((lead + n) * size + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
                out = raw[lead * size:(lead + n) * size].view(dt).view(nb, 12, N, N)
                fn, x = ((gogame.batch_move_planes, st), (gogame.batch_move_planes_tracked, tracked))[k % 2]
                assert fn(x[sl], dtype=dt, out=out) is out
                same(out.to(torch.uint8), c.planes[sl], tag)
                assert bool((raw[:lead * size] == SENTINEL).all()) and bool((raw[(lead + n) * size:] == SENTINEL).all()), tag
                same(gogame.batch_move_counts(st[sl]), c.counts[sl], tag + ('counts',))


def test_empty_batch():
    import torch
    from gymgo_amd import gogame
    for N in (2, 9, 13, 19):
        empty = torch.empty((0, 6, N, N), dtype=torch.uint8, device='cuda')
        none = torch.empty(0, dtype=torch.int32, device='cuda')
        assert tuple(gogame.batch_move_planes(empty).shape) == (0, 12, N, N)
        assert tuple(gogame.batch_move_planes(empty, dtype=torch.float32, orient=none).shape) == (0, 12, N, N)
        assert tuple(gogame.batch_move_counts(empty).shape) == (0, 3, N, N)
        tracked = torch.empty((0, 5 * N + 1), dtype=torch.int32, device='cuda')
        assert tuple(gogame.batch_move_planes_tracked(tracked).shape) == (0, 12, N, N)


def test_crafted_boards():
    import torch
    from gymgo_amd import gogame
    by_name = {}
    for N, (names, s) in sorted(oe.crafted_by_size().items()):
        raw = oe.batch_outcome(s)
        st = mc.to_dev(s)
        counts = gogame.batch_move_counts(st)
        same(counts, oe.counts_of(raw), (N, 'counts'))
        same(gogame.batch_move_planes(st), oe.planes_of(raw), (N, 'planes'))
        same(gogame.batch_move_planes_tracked(gogame.batch_track(st), dtype=torch.bfloat16).to(torch.uint8), oe.planes_of(raw), (N, 'tracked'))
        for name, row in zip(names, mc.to_np(counts)):
            by_name[name] = row
    for name, s, checks in oe.CRAFTED:       # ... and what each board was drawn for, from the device's bytes
        for y, x, want in checks:
            assert tuple(int(v) for v in by_name[name][:, y, x]) == tuple(min(v, 255) for v in want), (name, y, x)
    one = oe.CRAFTED[0][1]                    # the single-state forms, NumPy in and out
    raw = oe.outcome(one)
    got = gogame.move_planes(one, dtype=torch.float32)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, oe.planes_of(raw).astype(np.float32))
    assert np.array_equal(gogame.move_counts(one), oe.counts_of(raw))
    assert len(gogame.MOVE_NAMES) == gogame.MOVE_PLANES == 12 and gogame.MOVE_NAMES == oe.NAMES


def test_argument_errors():
    import torch
    from gymgo_amd import gogame
    from gymgo_amd._lib import GymGoNativeError
    N = 5
    st = mc.to_dev(oe.CRAFTED[0][1][None])
    tracked = gogame.batch_track(st)
    for bad in (torch.float64, torch.int32, np.uint8, None):
        with pytest.raises(ValueError):
            gogame.batch_move_planes(st, dtype=bad)
        with pytest.raises(ValueError):
            gogame.batch_move_planes_tracked(tracked, dtype=bad)
    with pytest.raises(GymGoNativeError):
        gogame.batch_move_planes(st.cpu())                                    # a host tensor never computes
    with pytest.raises(GymGoNativeError):
        gogame.batch_move_planes_tracked(tracked.cpu())
    with pytest.raises(GymGoNativeError):
        gogame.batch_move_counts(st.cpu())
    with pytest.raises(ValueError):
        gogame.batch_move_planes(st[:, :5])
    with pytest.raises(ValueError):
        gogame.batch_move_planes(st, orient=[0, 1])
    with pytest.raises(ValueError):
        gogame.batch_move_planes(st, out=torch.empty((1, 12, N, N), dtype=torch.float16, device='cuda'))
    with pytest.raises(ValueError):
        gogame.batch_move_planes(st.cpu().numpy(), dtype=torch.bfloat16)
    E = tsio.on_device(tsio.point_evaluator)
    for call in (lambda: gogame.PuctSearch(st, 3, outcome=True), lambda: gogame.batch_puct(st, 3, E, outcome=True),
                 lambda: gogame.puct_play(st, 1, 3, E, outcome=True), lambda: gogame.puct_selfplay(st, 1, 3, E, outcome=True),
                 lambda: gogame.puct(st[0], 3, E, outcome=True), lambda: gogame.puct_actions(st, 3, E, outcome=True)):
        with pytest.raises(ValueError, match='outcome=True'):
            call()


# ---------------------------------------------------------------- the search
def outcome_roots(N):
    """tsio.roots7 with the first root replaced by the running policy game with the most capturing points."""
    roots = tsio.roots7(N).copy()
    c = oe.case(N, 'policy')
    weight = c.planes[:, 4:8].reshape(B, -1).sum(axis=1) * (c.states[:, 5, 0, 0] == 0)
    best = int(np.argmax(weight))
    assert weight[best] > 0
    roots[0] = c.states[best]
    return roots


@pytest.mark.parametrize('life,ladder', [(False, False), (True, True)])
def test_search_hands_out_the_outcome_planes_of_its_leaves(life, ladder):
    import torch
    from gymgo_amd import gogame
    N, leaves, rounds = 5, 2, 4
    roots = mc.to_dev(outcome_roots(N))
    E = tsio.on_device(tsio.point_evaluator)
    ignore = lambda planes, legal, *more: E(planes, legal)
    kw = dict(komi=0.5, leaves=leaves, features=torch.float16, symmetry=99)
    sa = gogame.PuctSearch(roots, rounds, life=life, ladder=ladder, outcome=True, **kw)
    sb = gogame.PuctSearch(roots, rounds, komi=0.5, leaves=leaves)              # the states of the same leaves
    seen = False
    for t in range(rounds):
        res = sa.select()
        assert len(res) == 3 + life + ladder
        planes, legal, out = res[0], res[1], res[-1]
        states, _ = sb.select()
        assert out.dtype == torch.float16 and tuple(out.shape) == (7 * leaves, 12, N, N)
        o = mc.to_np(sa.orient)
        assert len(set(o & 7)) > 1
        same(out.to(torch.uint8), pc.turned(oe.batch_planes(mc.to_np(states)), o), (t, 'against the expectation'))
        assert bool((out.to(torch.uint8) == gogame.batch_move_planes(states, orient=sa.orient)).all()), t
        if ladder:
            assert bool((res[-2].to(torch.uint8) == gogame.batch_ladder(states, orient=sa.orient)).all()), t
        seen = seen or bool(out[:, 4:8].any())
        priors, values = E(planes, legal)
        sa.backup(priors, values)
        sb.backup(gogame.batch_symmetry_policy(priors, sa.orient, inverse=True), values)
    assert seen
    # the tree is the tree of the search without outcome, given an evaluator that ignores the extra planes
    a = gogame.batch_puct(roots, rounds, ignore, tree=True, life=life, ladder=ladder, outcome=True, **kw)
    b = gogame.batch_puct(roots, rounds, E, tree=True, **kw)
    tgf.same_tuples(a, b, (life, ladder))
    tgf.same_tuples(sa.result(tree=True), a, (life, ladder, 'steps'))


def test_selfplay_batch_with_outcome():
    import torch
    from gymgo_amd import gogame
    N, M, T, R = 5, 4, 4, 7
    roots = mc.to_dev(outcome_roots(N))
    kw = dict(c=0.6, komi=0.5, leaves=2, capacity=64, sample_moves=2, seed=7, features=torch.float16, record_states=True)
    calls = []

    def ignore(planes, legal, out):
        calls.append(tuple(out.shape))
        return tsio.on_device(tsio.point_evaluator)(planes, legal)

    a = gogame.puct_selfplay(roots, M, T, ignore, outcome=True, **kw)
    b = gogame.puct_selfplay(roots, M, T, tsio.on_device(tsio.point_evaluator), **kw)
    tgf.same_tuples(a, b)
    assert len(calls) == M * T and calls[0] == (R * 2, 12, N, N)
    games, moves = np.repeat(np.arange(R), M), np.tile(np.arange(M), R)
    orient = mixed(R * M)
    five = gogame.selfplay_batch(a, games, moves, orient, outcome=True)
    seven = gogame.selfplay_batch(a, games, moves, orient, life=True, ladder=True, outcome=True)
    four = gogame.selfplay_batch(a, games, moves, orient)
    assert len(five) == 5 and len(seven) == 7 and len(four) == 4 and all(torch.equal(x, y) for x, y in zip(five, four))
    st = mc.to_np(a.states)[games, moves]
    want = pc.turned(oe.batch_planes(st), orient)
    assert five[4].dtype == torch.float16 and torch.equal(five[4], seven[6])
    same(five[4].to(torch.uint8), want, 'outcome')
    same(gogame.selfplay_batch(a, games, moves, orient, dtype=torch.uint8, outcome=True)[4], want, 'uint8')
    same(five[4].to(torch.uint8), mc.to_np(gogame.batch_move_planes(mc.to_dev(st), orient=orient)), 'batch_move_planes of the recorded positions')
    assert want.any()
