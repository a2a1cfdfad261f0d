"""-m gpu: the pass-alive life planes (gogame.batch_life / batch_life_tracked / batch_settled: k_life of gg_life.h) - every
byte equal to the definitional expectation (tests/life_expect.py): positions of the no_eye_fill policy of every board-size
class at three depths with a ragged last wave, the crafted boards (the cascade that needs one pass per chain next to boards
that need one, the spiral, the comb, the row wrap, full boards), slices at any element offset between sentinels, the four
dtypes, the eight orientations, tracked input against byte planes also after plies on the tracked boards, out=, settled
on and off, a stream, NumPy, B = 0; and PuctSearch / batch_puct / puct_selfplay / selfplay_batch with life=True."""
import functools

import numpy as np
import pytest

import features_expect as fe
import life_expect as le
import mc_expect as mc
import mc_policy_expect as mp
import test_gpu_features as tgf
import test_gpu_symmetry_io as tsio

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 5, 9, 13, 19)
SENTINEL = 0xA5
same = tgf.same


def batch_of(N):
    return 65 if N == 19 else 257     # one board in the last wave: two boards per wave at 19x19, four below


@functools.lru_cache(maxsize=None)
def positions(N):
    """Positions of the no_eye_fill policy from the empty board (CPU, auto_reset off), a third of the boards each after N^2,
    3 N^2 / 2 and 2 N^2 plies -> (NumPy states, planes, settled, the slices of the three depths), computed once."""
    B = batch_of(N)
    cur, rng = np.zeros((B, 6, N, N), np.uint8), mc.po_seed(7 + N, np.arange(B))
    cuts = [0, B // 3, 2 * B // 3, B]
    out, done = np.zeros_like(cur), 0
    for i, depth in enumerate((N * N, 3 * N * N // 2, 2 * N * N)):
        cur, rng, _, _ = mp.policy_rollout(cur, rng, depth - done, auto_reset=False)
        done = depth
        out[cuts[i]:cuts[i + 1]] = cur[cuts[i]:cuts[i + 1]]
    planes = le.batch_life(out)
    return out, planes, le.settled_of(planes), [slice(cuts[i], cuts[i + 1]) for i in range(3)]


@functools.lru_cache(maxsize=None)
def crafted(N):
    parts = [le.small_boards()] if N == 5 else [le.crafted(N), fe.crafted(N)]     # (the cascade first: the tests index it)
    s = np.concatenate(parts + [mc.crafted_roots(N)])
    planes = le.batch_life(s)
    return s, planes, le.settled_of(planes)


def mixed(B):
    """All eight orientations in every wave, with negative and large words (only o & 7 is read)."""
    o = (np.arange(B, dtype=np.int64) * 3 + 1) % 8
    o[1::5] -= 8
    o[2::7] += 0x7FFFFFF8
    o[3::11] -= 0x80000000
    return o.astype(np.int32)


@pytest.mark.parametrize('N', SIZES)
def test_policy_positions_planes_and_settled(N):
    import torch
    from gymgo_amd import gogame
    s, planes, settled, depths = positions(N)
    B = batch_of(N)
    if N >= 5:   # not vacuous: asserted on the expectation
        mid = planes[depths[1]]
        assert 2 * int((mid[:, 0] | mid[:, 1]).any(axis=(1, 2)).sum()) >= len(mid), N
        assert settled.any() and not settled.all(), N
    st = mc.to_dev(s)
    got, flags = gogame.batch_life(st, settled=True)
    assert got.dtype == torch.uint8 and flags.dtype == torch.uint8
    same(got, planes, N)
    same(flags, settled, N)
    same(gogame.batch_life(st), planes, (N, 'settled=NULL'))
    same(gogame.batch_settled(st), settled, N)
    tracked = gogame.batch_track(st)
    got, flags = gogame.batch_life_tracked(tracked, settled=True)
    same(got, planes, (N, 'tracked'))
    same(flags, settled, (N, 'tracked'))
    # a lone board and a wave that is not full, at three offsets into a larger buffer: for odd N in uint8 a slice starts and
    # ends at any byte - the two ragged ends of the wave's slice, with sentinels before and after out and settled
    from gymgo_amd import _lib
    P4 = 4 * N * N
    for dt, size in ((torch.uint8, 1), (torch.float16, 2)):
        code = gogame._feature_dtype(dt)
        for nb in (1, 3):
            for k, first in enumerate((0, 100 % (B - nb), B - nb)):
                lead = (1, 7, 20)[k]                      # elements in front of out
                raw = torch.full(((lead + nb * P4) * size + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
                out = raw[lead * size:(lead + nb * P4) * size].view(dt).view(nb, 4, N, N)
                fraw = torch.full((nb + 9,), SENTINEL, dtype=torch.uint8, device='cuda')
                name, fn, x = (('gg_batch_life', gogame.batch_life, st), ('gg_batch_life_tracked', gogame.batch_life_tracked, tracked))[k % 2]
                xs = x[first:first + nb]
                _lib.check(getattr(_lib.lib(), name)(xs.data_ptr(), None, out.data_ptr(), fraw[3:].data_ptr(), code, nb, N,
                                                     _lib.stream_ptr(st.device)), name)
                same(out.to(torch.uint8), planes[first:first + nb], (N, dt, nb, first))
                same(fraw[3:3 + nb], settled[first:first + nb], (N, dt, nb, first))
                assert bool((raw[:lead * size] == SENTINEL).all()) and bool((raw[(lead + nb * P4) * size:] == SENTINEL).all())
                assert bool((fraw[:3] == SENTINEL).all()) and bool((fraw[3 + nb:] == SENTINEL).all())
                out.zero_()
                assert fn(xs, dtype=dt, out=out) is out                   # ... and through the Python call
                same(out.to(torch.uint8), planes[first:first + nb], (N, dt, nb, first, 'out='))
                assert bool((raw[:lead * size] == SENTINEL).all()) and bool((raw[(lead + nb * P4) * size:] == SENTINEL).all())


@pytest.mark.parametrize('N', (5, 9, 19))
def test_crafted_boards_and_the_cascade_next_to_one_pass_boards(N):
    import torch
    from gymgo_amd import gogame
    s, planes, settled = crafted(N)
    if N >= 9:   # what the boards are there for: all alive / all dead after one iteration per chain
        L = (N - 2) // 3 + 1
        assert np.array_equal(planes[0, 0], s[0, 0]) and not planes[4].any() and le.iterations(s[4]) == L >= 3
    st = mc.to_dev(s)
    got, flags = gogame.batch_life(st, settled=True)
    same(got, planes, N)
    same(flags, settled, N)
    same(gogame.batch_life_tracked(gogame.batch_track(st)), planes, (N, 'tracked'))
    for i in (0, 4, len(s) - 1):
        same(gogame.life(st[i]), planes[i], (N, i))
    if N < 9:
        return
    # every wave holds a board that needs a pass per chain next to boards that need one
    pos = positions(N)
    reps = 9
    idx = np.concatenate([[4 + (k % 4)] + [len(s) + 3 * k + j for j in range(3)] for k in range(reps)])
    alls, allp = np.concatenate([s, pos[0]]), np.concatenate([planes, pos[1]])
    same(gogame.batch_life(mc.to_dev(alls[idx])), allp[idx], (N, 'tiled'))
    same(gogame.batch_life(mc.to_dev(alls[idx[::-1]].copy()), dtype=torch.float16).to(torch.uint8), allp[idx[::-1]], (N, 'tiled'))


@pytest.mark.parametrize('N', (3, 5, 13, 19))
def test_dtypes(N):
    import torch
    from gymgo_amd import gogame
    s, planes, settled, _ = positions(N)
    st = mc.to_dev(s)
    tracked = gogame.batch_track(st)
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        got, flags = gogame.batch_life(st, dtype=dt, settled=True)
        assert got.dtype == dt and tuple(got.shape) == planes.shape
        assert bool(((got == 0) | (got == 1)).all())
        same(got.to(torch.uint8), planes, (N, dt))
        same(flags, settled, (N, dt))
        same(gogame.batch_life_tracked(tracked, dtype=dt).to(torch.uint8), planes, (N, dt, 'tracked'))
    assert gogame.batch_life(st).dtype == torch.uint8          # the default


@pytest.mark.parametrize('N', SIZES)
def test_tracked_input_also_after_plies(N):
    import torch
    from gymgo_amd import gogame
    s, planes, _, _ = positions(N)
    B = batch_of(N)
    st = mc.to_dev(s)
    tracked = gogame.batch_track(st)
    rng = gogame.rng_seed(B, 77 + N)
    for ply in range(5):
        acts = gogame.batch_sample_actions(gogame.batch_untrack(tracked), rng)
        gogame.batch_play_moves_tracked(tracked, acts[:, None])
        if ply in (0, 4):
            now = gogame.batch_untrack(tracked)
            got, flags = gogame.batch_life_tracked(tracked, settled=True)
            g2, f2 = gogame.batch_life(now, settled=True)
            assert bool((got == g2).all()) and bool((flags == f2).all()), (N, ply)
            sub = slice(None, None, 8 if N >= 13 else 4)
            want = le.batch_life(now[sub].cpu().numpy())
            same(got[sub], want, (N, ply))
            same(flags[sub], le.settled_of(want), (N, ply))
    assert not bool((now == st).all())


@pytest.mark.parametrize('N', SIZES)
def test_orientations(N):
    import torch
    from gymgo_amd import gogame
    s, planes, settled, _ = positions(N)
    B = batch_of(N)
    st = mc.to_dev(s)
    tracked = gogame.batch_track(st)
    for orient in (mixed(B), (np.arange(B) % 4).astype(np.int32)):     # ... and a batch none of whose boards rotates
        want = le.oriented(planes, orient)
        got, flags = gogame.batch_life(st, orient=orient, settled=True)
        same(got, want, N)
        same(flags, settled, N)                                          # settled does not turn
        same(gogame.batch_life_tracked(tracked, orient=torch.from_numpy(orient).cuda()), want, (N, 'tracked'))
        o8 = torch.from_numpy(orient & 7).cuda()
        same(gogame.batch_symmetry(gogame.batch_life(st), o8), want, (N, 'batch_symmetry of the planes'))
        same(gogame.batch_life(gogame.batch_symmetry(st, o8)), want, (N, 'the planes of the turned position'))
    same(gogame.batch_life(st, dtype=torch.float32, orient=mixed(B)).to(torch.uint8), le.oriented(planes, mixed(B)), (N, 'f32'))


def test_plumbing_out_stream_numpy_and_empty_batch():
    import torch
    from gymgo_amd import gogame
    N = 9
    s, planes, settled, _ = positions(N)
    B = batch_of(N)
    st = mc.to_dev(s)
    tracked = gogame.batch_track(st)
    out = torch.empty((B, 4, N, N), dtype=torch.float16, device='cuda')
    assert gogame.batch_life(st, dtype=torch.float16, out=out) is out
    same(out.to(torch.uint8), planes)
    out.zero_()
    assert gogame.batch_life_tracked(tracked, dtype=torch.float16, out=out, settled=True)[0] is out
    same(out.to(torch.uint8), planes)
    with pytest.raises(ValueError):
        gogame.batch_life(st, dtype=torch.float32, out=out)
    with pytest.raises(ValueError):
        gogame.batch_life(st, dtype=torch.float16, out=out[:, :, :, :-1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = gogame.batch_life(st, orient=mixed(B))
        b, f = gogame.batch_life_tracked(tracked, settled=True)
    side.synchronize()
    same(a, le.oriented(planes, mixed(B)))
    same(b, planes)
    same(f, settled)
    got, flags = gogame.batch_life(s, settled=True)                       # NumPy in, NumPy out
    assert isinstance(got, np.ndarray) and isinstance(flags, np.ndarray)
    same(got, planes)
    same(flags, settled)
    assert isinstance(gogame.batch_settled(s), np.ndarray)
    got = gogame.batch_life(s[:5], dtype=torch.float32, orient=list(mixed(5)))
    assert got.dtype == np.float32 and np.array_equal(got, le.oriented(planes[:5], mixed(5)).astype(np.float32))
    one, flag = gogame.life(s[3], settled=True)
    assert np.array_equal(one, planes[3]) and int(flag) == settled[3]
    empty = torch.empty((0, 6, N, N), dtype=torch.uint8, device='cuda')
    none = torch.empty(0, dtype=torch.int32, device='cuda')
    got, flags = gogame.batch_life(empty, orient=none, settled=True)
    assert tuple(got.shape) == (0, 4, N, N) and tuple(flags.shape) == (0,)
    assert tuple(gogame.batch_life_tracked(tracked[:0]).shape) == (0, 4, N, N)
    assert tuple(gogame.batch_settled(empty).shape) == (0,)


# ---------------------------------------------------------------- the search
def life_evaluator(planes, legal, life):
    """tsio.point_evaluator with the value shifted by the share of the points the life planes decide for either side."""
    priors, values = tsio.point_evaluator(planes, legal)
    lf = np.asarray(life).astype(np.float32)
    N = lf.shape[-1]
    shift = ((lf[:, 0] + lf[:, 2]).sum(axis=(1, 2), dtype=np.float32) - (lf[:, 1] + lf[:, 3]).sum(axis=(1, 2), dtype=np.float32))
    return priors, np.clip(values + shift / np.float32(2 * N * N), -1, 1).astype(np.float32)


def on_device3(E):
    import torch

    def evaluate(planes, legal, life):
        priors, values = E(planes.to(torch.float32).cpu().numpy(), legal.cpu().numpy(), life.to(torch.float32).cpu().numpy())
        return torch.from_numpy(priors).cuda(), torch.from_numpy(values).cuda()

    return evaluate


def settled_roots(N):
    """tsio.roots7 with the first root replaced by a running policy game whose life planes are not empty."""
    roots = tsio.roots7(N).copy()
    s, planes, _, _ = positions(N)
    weight = planes.reshape(len(planes), -1).sum(axis=1) * (s[:, 5, 0, 0] == 0)     # (an ended root's evaluation is ignored)
    best = int(np.argmax(weight))
    assert planes[best].any() and not s[best, 5].any()
    roots[0] = s[best]
    return roots


@pytest.mark.parametrize('N,leaves,rounds', [(5, None, 5), (5, 3, 5), (9, None, 5), (9, 3, 5), (19, 4, 3)])
def test_search_hands_out_the_life_planes_of_its_leaves(N, leaves, rounds):
    import torch
    from gymgo_amd import gogame
    roots = mc.to_dev(settled_roots(N))
    ignore = lambda planes, legal, life: tsio.on_device(tsio.point_evaluator)(planes, legal)
    for symmetry in (None, 99 + N):
        kw = dict(komi=0.5, leaves=leaves, features=torch.float16, symmetry=symmetry)
        sa = gogame.PuctSearch(roots, rounds, life=True, **kw)
        sb = gogame.PuctSearch(roots, rounds, komi=0.5, leaves=leaves)          # the states of the same leaves
        E = tsio.on_device(tsio.point_evaluator)
        seen = False
        for t in range(rounds):
            planes, legal, life = sa.select()
            states, _ = sb.select()
            assert life.dtype == torch.float16 and tuple(life.shape) == (states.shape[0], 4, N, N)
            want = gogame.batch_life(states, dtype=torch.uint8, orient=None if symmetry is None else sa.orient)
            assert bool((life.to(torch.uint8) == want).all()), (N, leaves, symmetry, t)
            if t in (0, rounds - 1):     # ... and against the expectation itself
                w = le.batch_life(mc.to_np(states))
                same(life.to(torch.uint8), w if symmetry is None else le.oriented(w, mc.to_np(sa.orient)), (N, leaves, symmetry, t))
            seen = seen or bool(life.any())
            priors, values = E(planes, legal)
            sa.backup(priors, values)
            sb.backup(priors if symmetry is None else gogame.batch_symmetry_policy(priors, sa.orient, inverse=True), values)
        assert seen
        # the tree is the tree of the search without life, given an evaluator that ignores its third argument
        a = gogame.batch_puct(roots, rounds, ignore, tree=True, life=True, **kw)
        b = gogame.batch_puct(roots, rounds, E, tree=True, **kw)
        tgf.same_tuples(a, b, (N, leaves, symmetry))
        tgf.same_tuples(sa.result(tree=True), a, (N, leaves, symmetry, 'steps'))
    # an evaluator that reads the planes changes the tree
    c = gogame.batch_puct(roots, rounds, on_device3(life_evaluator), tree=True, life=True, komi=0.5, leaves=leaves, features=torch.float16)
    plain = gogame.batch_puct(roots, rounds, E, tree=True, komi=0.5, leaves=leaves, features=torch.float16)
    assert not bool((c.tree.value_sum == plain.tree.value_sum).all())


@pytest.mark.parametrize('leaves', (None, 2))
def test_selfplay_with_life_and_selfplay_batch(leaves):
    import torch
    from gymgo_amd import gogame
    N, M, T = 5, 5, 6
    roots = mc.to_dev(settled_roots(N))
    R = 7
    kw = dict(c=0.6, komi=0.5, leaves=leaves, capacity=64, sample_moves=2, seed=7, features=torch.float16, record_states=True)
    calls = []

    def ignore(planes, legal, life):
        calls.append(tuple(life.shape))
        return tsio.on_device(tsio.point_evaluator)(planes, legal)

    a = gogame.puct_selfplay(roots, M, T, ignore, life=True, **kw)
    b = gogame.puct_selfplay(roots, M, T, tsio.on_device(tsio.point_evaluator), **kw)
    tgf.same_tuples(a, b, leaves)
    assert len(calls) == M * T and calls[0] == (R * (leaves or 1), 4, N, N)
    games, moves = np.repeat(np.arange(R), M), np.tile(np.arange(M), R)
    orient = mixed(R * M)
    five = gogame.selfplay_batch(a, games, moves, orient, life=True)
    four = gogame.selfplay_batch(a, games, moves, orient)
    assert len(five) == 5 and len(four) == 4 and all(torch.equal(x, y) for x, y in zip(five, four))
    st = mc.to_np(a.states)[games, moves]
    assert five[4].dtype == torch.float16
    same(five[4].to(torch.uint8), le.oriented(le.batch_life(st), orient), 'life')
    same(gogame.selfplay_batch(a, games, moves, orient, dtype=torch.uint8, life=True)[4], le.oriented(le.batch_life(st), orient), 'uint8')
    assert le.batch_life(st).any()
