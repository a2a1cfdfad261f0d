"""-m gpu: the symmetry-aware network I/O (k_features_oriented of gg_feat.h, k_symmetry_policy of gg_sym.h, k_draw_orient)
against tests/symmetry_expect.py.  Planes: the positions of test_gpu_features.py (every kernel layout, ragged waves, ended
games, crafted boards with either colour to move) with all eight orientations mixed in every wave and with no rotation at
all, byte for byte against the oriented expectation, against gg_batch_symmetry of the plain planes and against the planes of
the turned position; tracked against byte-plane input; the four dtypes; out=, a stream, NumPy, B = 0, a sentinel behind out.
The policy turn: three element sizes, NaN bit patterns, misaligned slices, sentinels around out.  The draw.  The search:
PuctSearch(symmetry=) against the plain search with the wrapped evaluator, field by field as bit patterns, in shards, through
puct_selfplay, and selfplay_batch on its record."""
import numpy as np
import pytest

import features_expect as fe
import mc_expect as mc
import mc_puct_selfplay_expect as ps
import symmetry_expect as se
import test_gpu_features as tgf
import test_gpu_puct_selfplay as tps

pytestmark = pytest.mark.gpu

B_RANDOM = tgf.B_RANDOM
SENTINEL = 0xA5


def same(got, want, tag=''):
    tgf.same(got, want, tag)


def mixed(B):
    return np.arange(B, dtype=np.int32) % 8


# ---------------------------------------------------------------- planes
@pytest.mark.parametrize('N', tgf.SIZES)
def test_oriented_planes(N):
    import torch
    from gymgo_amd import gogame
    st, s, planes, _ = tgf.positions(N)
    ended = s[:, 5, 0, 0] != 0
    assert ended.any() and not ended.all()
    tracked = gogame.batch_track(st)
    plain = mc.to_dev(planes)
    for orient in (mixed(B_RANDOM), mixed(B_RANDOM) % 4, np.where(np.arange(B_RANDOM) % 3 == 0, -(mixed(B_RANDOM) + 40), mixed(B_RANDOM) + 40)):
        want = se.orient_images(planes, orient)          # (only orient & 7 is read: negative and large values too)
        o = torch.from_numpy(orient.astype(np.int32)).cuda()
        got = gogame.batch_features(st, dtype=torch.uint8, orient=o)
        same(got, want, (N, 'bytes'))
        same(gogame.batch_features_tracked(tracked, dtype=torch.uint8, orient=o), want, (N, 'tracked'))
        assert bool((got == gogame.batch_symmetry(plain, o & 7)).all())                                     # the planes turned as an image
        assert bool((got == gogame.batch_features(gogame.batch_symmetry(st, o & 7), dtype=torch.uint8)).all())   # the planes of the turned position
        assert bool((got == gogame.batch_features_tracked(gogame.batch_symmetry_rows(tracked, N, o & 7), dtype=torch.uint8)).all())
    assert not np.array_equal(se.orient_images(planes, mixed(B_RANDOM)), planes)
    orient = mixed(B_RANDOM)
    want = se.orient_images(planes, orient)
    for B in (1, 3):        # a lone board, a wave that is not full; slices that start at any byte
        for first in (0, 100, B_RANDOM - B):
            sl = slice(first, first + B)
            a = gogame.batch_features(st[sl], dtype=torch.uint8, orient=orient[sl])
            b = gogame.batch_features_tracked(tracked[sl], dtype=torch.uint8, orient=orient[sl])
            same(a, want[sl], (N, B, first))
            same(b, want[sl], (N, B, first, 'tracked'))


@pytest.mark.parametrize('N', (9, 19))
def test_oriented_crafted_boards(N):
    import torch
    from gymgo_amd import gogame
    s, planes, _ = tgf.crafted(N)
    assert (s[:, 2, 0, 0] == 0).any() and (s[:, 2, 0, 0] != 0).any()          # both colours to move
    st = mc.to_dev(s)
    for shift in range(8):                                                  # every board in every orientation
        orient = (mixed(len(s)) + shift) % 8
        want = se.orient_images(planes, orient)
        same(gogame.batch_features(st, dtype=torch.uint8, orient=orient), want, (N, shift))
        same(gogame.batch_features_tracked(gogame.batch_track(st), dtype=torch.uint8, orient=orient), want, (N, shift, 'tracked'))
    assert se.orient_images(planes, mixed(len(s)))[:, 11].sum() == planes[:, 11].sum() >= 1      # the ko point moves with the board


@pytest.mark.parametrize('N', (5, 13, 19))
def test_oriented_dtypes(N):
    import torch
    from gymgo_amd import gogame
    st, s, planes, _ = tgf.positions(N)
    orient = mixed(B_RANDOM)
    want = se.orient_images(planes, orient)
    tracked = gogame.batch_track(st)
    for dt in (torch.uint8, torch.float16, torch.bfloat16, torch.float32):
        got = gogame.batch_features(st, dtype=dt, orient=orient)
        assert got.dtype == dt and tuple(got.shape) == planes.shape
        assert bool(((got == 0) | (got == 1)).all())
        same(got.to(torch.uint8), want, (N, dt))
        same(gogame.batch_features_tracked(tracked, dtype=dt, orient=orient).to(torch.uint8), want, (N, dt, 'tracked'))
    assert gogame.batch_features(st, orient=orient).dtype == torch.float16


def test_oriented_plumbing_out_sentinel_stream_numpy_and_empty_batch():
    import torch
    from gymgo_amd import gogame
    N = 9
    st, s, planes, _ = tgf.positions(N)
    orient = mixed(B_RANDOM)
    want = se.orient_images(planes, orient)
    tracked = gogame.batch_track(st)
    n = B_RANDOM * 16 * N * N
    for dt, size in ((torch.uint8, 1), (torch.float16, 2), (torch.float32, 4)):
        for fn, x in ((gogame.batch_features, st), (gogame.batch_features_tracked, tracked)):
            raw = torch.full((n * size + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
            out = raw[:n * size].view(dt).view(B_RANDOM, 16, N, N)
            assert fn(x, dtype=dt, out=out, orient=orient) is out
            same(out.to(torch.uint8), want, (dt, fn.__name__))
            assert bool((raw[n * size:] == SENTINEL).all())                 # nothing behind out is written
    with pytest.raises(ValueError):
        gogame.batch_features(st, dtype=torch.float16, out=out, orient=orient)      # the wrong dtype
    # the last wave is ragged at every size: one board, and boards that end inside a wave, leave the bytes behind them alone
    for B in (1, 2, 3, 5):
        raw = torch.full((B * 16 * N * N + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
        out = raw[:B * 16 * N * N].view(B, 16, N, N)
        gogame.batch_features_tracked(tracked[:B], dtype=torch.uint8, out=out, orient=orient[:B])
        same(out, want[:B], B)
        assert bool((raw[B * 16 * N * N:] == SENTINEL).all())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = gogame.batch_features(st, dtype=torch.uint8, orient=orient)
        b = gogame.batch_features_tracked(tracked, dtype=torch.uint8, orient=torch.from_numpy(orient).to(torch.int64))
    side.synchronize()
    same(a, want)
    same(b, want)
    got = gogame.batch_features(s, dtype=torch.uint8, orient=list(orient))          # NumPy in, NumPy out
    assert isinstance(got, np.ndarray)
    same(got, want)
    got = gogame.batch_features(s[:5], dtype=torch.float32, orient=orient[:5])
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, want[:5].astype(np.float32))
    empty = torch.empty((0, 6, N, N), dtype=torch.uint8, device='cuda')
    none = torch.empty(0, dtype=torch.int32, device='cuda')
    assert tuple(gogame.batch_features(empty, orient=none).shape) == (0, 16, N, N)
    assert tuple(gogame.batch_features_tracked(tracked[:0], orient=none).shape) == (0, 16, N, N)


# ---------------------------------------------------------------- vectors over the actions
def policy_rows(B, A, size):
    """Rows of distinct bit patterns as an unsigned array (uint8: distinct as far as a byte goes); NaNs among the 32-bit ones."""
    b, a = np.arange(B, dtype=np.int64)[:, None], np.arange(A, dtype=np.int64)[None, :]
    if size == 1:
        return ((a * 31 + b * 7) % 251).astype(np.uint8)
    if size == 2:
        return ((a * 7 + b * 13 + 0x7C00 - 100) % 65536).astype(np.uint16)      # (float16 infinities and NaNs among them)
    x = (a * 2654435761 + b * 40503) % (2 ** 32)
    x = np.where(a % 5 == 1, 0x7FC00000 + a + 1000 * b, x)                       # quiet NaNs with payloads
    x = np.where(a % 5 == 2, 0xFF800001 + a, x)                                  # signalling NaNs, negative
    return x.astype(np.uint32)


@pytest.mark.parametrize('N', (2, 5, 9, 13, 19))
def test_policy_turn(N):
    import torch
    from gymgo_amd import gogame
    A = N * N + 1
    kinds = ((torch.uint8, 1, torch.uint8), (torch.bool, 1, torch.uint8), (torch.float16, 2, torch.int16), (torch.bfloat16, 2, torch.int16),
             (torch.float32, 4, torch.int32), (torch.int32, 4, torch.int32))
    for B in (1, 3, 257):
        orient = (mixed(B) + 3) % 8 if B > 1 else np.array([5], np.int32)
        for dt, size, bits in kinds:
            rows = policy_rows(B, A, size)
            if dt == torch.bool:
                rows = rows & 1
            want_f, want_i = se.turn_policy(rows, orient), se.turn_policy(rows, orient, inverse=True)
            assert np.array_equal(se.turn_policy(want_f, orient, inverse=True), rows)
            # slices that start at odd rows of larger buffers: misaligned bases, sentinel rows before and after `out`
            src = torch.zeros((B + 2, A), dtype=bits, device='cuda')
            src[1:B + 1] = torch.from_numpy(rows.view({1: np.uint8, 2: np.int16, 4: np.int32}[size])).cuda()
            x = src.view(dt)[1:B + 1]
            assert x.data_ptr() % 16 != 0 or (A * size) % 16 == 0
            for inverse, want in ((False, want_f), (True, want_i)):
                room = torch.full(((B + 2) * A * size,), SENTINEL, dtype=torch.uint8, device='cuda')
                out = room.view(dt).view(B + 2, A)[1:B + 1]
                assert gogame.batch_symmetry_policy(x, orient, inverse=inverse, out=out) is out
                got = out.contiguous().view(bits).cpu().numpy().view(rows.dtype)
                assert np.array_equal(got, want), (N, B, dt, inverse, np.argwhere(got != want)[:6])
                edge = room.view(B + 2, A * size)
                assert bool((edge[0] == SENTINEL).all()) and bool((edge[B + 1] == SENTINEL).all()), (N, B, dt, inverse)
                assert np.array_equal(src[1:B + 1].cpu().numpy().view(rows.dtype), rows)   # the input is not changed
            there = gogame.batch_symmetry_policy(x, orient)
            assert there.dtype == dt and tuple(there.shape) == (B, A)
            back = gogame.batch_symmetry_policy(there, torch.from_numpy(orient).cuda(), inverse=True)
            assert bool((back.view(bits) == x.contiguous().view(bits)).all()), (N, B, dt)


def test_policy_turn_plumbing():
    import torch
    from gymgo_amd import gogame
    N, B = 9, 37
    A = N * N + 1
    orient = mixed(B)
    rows = policy_rows(B, A, 4)
    got = gogame.batch_symmetry_policy(rows.view(np.float32), orient)                          # NumPy in, NumPy out
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), se.turn_policy(rows, orient))
    got = gogame.batch_symmetry_policy((rows & 1).astype(bool), orient, inverse=True)
    assert got.dtype == np.bool_ and np.array_equal(got, se.turn_policy((rows & 1).astype(bool), orient, inverse=True))
    x = torch.from_numpy(rows.astype(np.int64)).cuda().to(torch.int32)
    want = se.turn_policy(mc.to_np(x), orient + 8)                                               # only orient & 7 is read
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y = gogame.batch_symmetry_policy(x, orient + 8)
    side.synchronize()
    assert np.array_equal(mc.to_np(y), want)
    assert tuple(gogame.batch_symmetry_policy(x[:0], orient[:0]).shape) == (0, A)
    with pytest.raises(ValueError):
        gogame.batch_symmetry_policy(x, orient, out=x)                                           # overlap
    with pytest.raises(ValueError):
        gogame.batch_symmetry_policy(x, orient, out=torch.empty((B, A), dtype=torch.float32, device='cuda'))


# ---------------------------------------------------------------- the draw
@pytest.mark.parametrize('B', (1, 65, 257))
def test_draw_orient(B):
    import torch
    from gymgo_amd import gogame
    rng = gogame.rng_seed(B, 99, 5)
    start = se.seeds(B, 99, 5)
    assert [int(v) for v in mc.to_np(rng).view(np.uint64)] == start
    for _ in range(3):
        got = gogame.batch_draw_orient(rng)
        want, start = se.draw_orient(start)
        assert got.dtype == torch.int32 and np.array_equal(mc.to_np(got), want)
        assert [int(v) for v in mc.to_np(rng).view(np.uint64)] == start
    assert tuple(gogame.batch_draw_orient(rng[:0]).shape) == (0,)


# ---------------------------------------------------------------- the search
def point_evaluator(planes, legal):
    """NumPy, defined on planes AND on the point index: priors proportional to (1 + 2 * capture plane) * (1 + (q mod 7) / 8)
    over the legal actions (the pass weighs 1), value = (own stones - opponent stones) / N^2 in float32.  Not symmetric: a
    turned board gets other priors."""
    p = np.asarray(planes).astype(np.float32)
    B, N = p.shape[0], p.shape[-1]
    q = (np.float32(1) + (np.arange(N * N) % 7).astype(np.float32) / np.float32(8))[None, :]
    w = np.concatenate([(np.float32(1) + np.float32(2) * p[:, 12].reshape(B, N * N)) * q, np.ones((B, 1), np.float32)], axis=1)
    w = np.where(legal, w, np.float32(0)).astype(np.float32)
    priors = w / np.maximum(w.sum(axis=1, keepdims=True, dtype=np.float32), np.float32(1))
    values = (p[:, 0].sum(axis=(1, 2), dtype=np.float32) - p[:, 1].sum(axis=(1, 2), dtype=np.float32)) / np.float32(N * N)
    return priors.astype(np.float32), values.astype(np.float32)


def on_device(E):
    """A NumPy evaluator as the search's evaluator: device tensors in and out."""
    import torch

    def evaluate(planes, legal):
        priors, values = E(planes.to(torch.float32).cpu().numpy(), legal.cpu().numpy())
        return torch.from_numpy(priors).cuda(), torch.from_numpy(values).cuda()

    return evaluate


def roots7(N):
    """7 roots: three of random play, the empty board, a root after a pass, a ko, a finished game."""
    roots = np.concatenate([mc.make_roots(N, 4, 50 + N, max_ply=N * N, step=N)[1:], mc.crafted_roots(N)])
    assert roots.shape[0] == 7 and (roots[:, 5, 0, 0] != 0).any()
    return roots


def cat_tuples(parts):
    import torch
    first = parts[0]
    return type(first)(*[None if getattr(first, k) is None else
                         cat_tuples([getattr(p, k) for p in parts]) if isinstance(getattr(first, k), tuple) else
                         torch.cat([getattr(p, k) for p in parts]) for k in first._fields])


def differs(a, b):
    return any(not bool((getattr(a, k) == getattr(b, k)).all()) for k in ('visits', 'prior'))


@pytest.mark.parametrize('N,leaves,rounds', [(5, None, 6), (5, 3, 6), (9, None, 6), (9, 3, 6), (19, 4, 3)])
def test_search_with_symmetry_is_the_plain_search_with_the_wrapped_evaluator(N, leaves, rounds):
    import torch
    from gymgo_amd import gogame
    roots = mc.to_dev(roots7(N))
    R, rows, seed = 7, leaves or 1, 424242 + N
    kw = dict(komi=0.5, tree=True, leaves=leaves, features=torch.float16)
    a = gogame.batch_puct(roots, rounds, on_device(point_evaluator), symmetry=seed, **kw)
    W = se.wrapped(point_evaluator, seed)
    b = gogame.batch_puct(roots, rounds, on_device(W), **kw)
    tgf.same_tuples(a, b, (N, leaves))
    assert len(W.orients) == rounds and len({tuple(o) for o in W.orients}) > 1 and all(len(o) == R * rows for o in W.orients)
    plain = gogame.batch_puct(roots, rounds, on_device(point_evaluator), **kw)
    assert differs(a, plain)                                    # else the comparison above shows nothing
    assert int(a.root_visits.sum()) > R
    # shards by root concatenate to the whole
    parts = [gogame.batch_puct(roots[:3], rounds, on_device(point_evaluator), symmetry=seed, **kw),
             gogame.batch_puct(roots[3:], rounds, on_device(point_evaluator), symmetry=seed, first_root=3, **kw)]
    tgf.same_tuples(cat_tuples(parts), a, (N, leaves, 'shards'))
    if N == 19:
        return
    # step by step beside the plain search: search.orient, the planes and legal in that view, the priors turned back
    sa = gogame.PuctSearch(roots, rounds, komi=0.5, leaves=leaves, features=torch.float16, symmetry=seed)
    sb = gogame.PuctSearch(roots, rounds, komi=0.5, leaves=leaves, features=torch.float16)
    E = on_device(point_evaluator)
    for t in range(rounds):
        pa, la = sa.select()
        pb, lb = sb.select()
        o = mc.to_np(sa.orient)
        assert sa.orient.dtype == torch.int32 and np.array_equal(o, W.orients[t]), t
        same(pa.to(torch.uint8), se.orient_images(mc.to_np(pb.to(torch.uint8)), o), (N, leaves, t))
        same(la, se.turn_policy(mc.to_np(lb), o), (N, leaves, t, 'legal'))
        priors, values = E(pa, la)
        sa.backup(priors, values)
        sb.backup(gogame.batch_symmetry_policy(priors, o, inverse=True), values)
    tgf.same_tuples(sa.result(tree=True), sb.result(tree=True), (N, leaves, 'steps'))
    tgf.same_tuples(sa.result(tree=True), a, (N, leaves, 'loop'))
    assert bool((gogame.puct_actions(roots, rounds, on_device(point_evaluator), komi=0.5, leaves=leaves, features=torch.float16, symmetry=seed)
                 == gogame.puct_actions(roots, rounds, on_device(se.wrapped(point_evaluator, seed)), komi=0.5, leaves=leaves,
                                        features=torch.float16)).all())


@pytest.mark.parametrize('leaves', (None, 2))
def test_selfplay_with_symmetry_and_selfplay_batch(leaves):
    import torch
    from gymgo_amd import gogame
    N, M, T, seed, first = 5, 5, 6, 77, 2
    roots = roots7(N)
    R, A, rows = 7, N * N + 1, leaves or 1
    kw = dict(c=0.6, komi=0.5, leaves=leaves, capacity=64, sample_moves=2, seed=7, first_game=first)
    W = se.wrapped(point_evaluator, seed, first_row=first * rows)
    e = ps.expected_selfplay(roots, M, T, lambda states, legal: W(fe.batch_features(states), legal), **kw)
    assert (e['lengths'] == M).any() and (e['lengths'] == 0).any()
    rec = gogame.puct_selfplay(mc.to_dev(roots), M, T, on_device(point_evaluator), features=torch.float16, symmetry=seed,
                               record_states=True, **kw)
    tps._check_selfplay(rec, e, ('symmetry', leaves))
    unturned = gogame.puct_selfplay(mc.to_dev(roots), M, T, on_device(point_evaluator), features=torch.float16, **kw)
    assert not torch.equal(unturned.pi, rec.pi)
    # training samples: every recorded position, orientations mixed
    games, moves = np.repeat(np.arange(R), M), np.tile(np.arange(M), R)
    orient = mixed(R * M)
    planes, pi, z, valid = gogame.selfplay_batch(rec, games, moves, orient)
    assert planes.dtype == torch.float16 and pi.dtype == torch.float32 and z.dtype == torch.float32 and valid.dtype == torch.bool
    st = e['states'][games, moves]
    same(planes.to(torch.uint8), se.orient_images(fe.batch_features(st), orient), 'planes')
    want_pi = se.turn_policy(e['pi'][games, moves], orient)
    assert np.array_equal(mc.to_np(pi).view(np.uint32), want_pi.view(np.uint32))
    out = e['outcome'][games].astype(np.float32)
    assert np.array_equal(mc.to_np(z), np.where(st[:, 2, 0, 0] != 0, -out, out))
    assert np.array_equal(mc.to_np(valid), moves < e['lengths'][games])
    assert mc.to_np(valid).any() and not mc.to_np(valid).all() and (mc.to_np(z) != 0).any()
    p8 = gogame.selfplay_batch(rec, torch.from_numpy(games).cuda(), torch.from_numpy(moves).cuda(), orient, dtype=torch.uint8)[0]
    same(p8, se.orient_images(fe.batch_features(st), orient), 'uint8')
