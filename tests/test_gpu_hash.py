"""-m gpu: the position and move hashes and positional superko (k_hash / k_move_hashes of gg_hash.h: gogame.batch_hash,
batch_move_hashes, batch_superko_moves, batch_forbid_repeats, their tracked forms, PositionHistory,
PuctSearch.forbid_repeats, puct_play / puct_selfplay with superko=True) at EVERY board size from 2 to 19, every word equal to
the definitional expectation (tests/hash_expect.py; tests/test_hash_host.py holds what this file relies on)."""
import numpy as np
import pytest

import flood_cases as fc
import hash_expect as he
import mc_expect as mc
import outcome_expect as oe
import plane_cases as pc
import test_gpu_features as tgf
import test_gpu_symmetry_io as tsio

pytestmark = pytest.mark.gpu

B = pc.B
SETS = ('policy', 'clean')
SENTINEL = 0x5A5A5A5A5A5A5A5A
same = tgf.same


def history_of(hashes, count):
    """a PositionHistory on the device with these entries [B, H] and counts [B]"""
    import torch
    from gymgo_amd import gogame
    hist = gogame.PositionHistory(hashes.shape[0], hashes.shape[1])
    hist.hashes.copy_(torch.from_numpy(np.ascontiguousarray(hashes, dtype=np.int64)))
    hist.count.copy_(torch.from_numpy(np.ascontiguousarray(count, dtype=np.int32)))
    return hist


@pytest.mark.parametrize('N', pc.SIZES)
def test_base_and_move_hashes_byte_planes_and_tracked(N):
    import torch
    from gymgo_amd import gogame
    for kind in SETS:
        c = he.case(N, kind)
        st = mc.to_dev(c.states.copy())         # (the cached arrays are read-only)
        tracked = gogame.batch_track(st)
        for name, x, base, moves in (('bytes', st, gogame.batch_hash, gogame.batch_move_hashes),
                                     ('tracked', tracked, gogame.batch_hash_tracked, gogame.batch_move_hashes_tracked)):
            got = base(x)
            assert got.dtype == torch.int64 and tuple(got.shape) == (B,)
            same(got, c.hashes, (N, kind, name, 'hash'))
            got = moves(x)
            assert got.dtype == torch.int64 and tuple(got.shape) == (B, N * N + 1)
            same(got, c.moves, (N, kind, name, 'move hashes'))


def test_single_state_forms():
    from gymgo_amd import gogame
    N = 5
    c = he.case(N, 'policy')
    b = int(np.argmax((c.moves != c.hashes[:, None]).sum(axis=1)))
    one = c.states[b].copy()
    got = gogame.position_hash(one)                       # NumPy in, NumPy out
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.shape == () and int(got) == int(c.hashes[b])
    got = gogame.move_hashes(one)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, c.moves[b])
    dev = mc.to_dev(one.copy())
    assert int(gogame.position_hash(dev)) == int(c.hashes[b]) and gogame.position_hash(dev).is_cuda
    same(gogame.move_hashes(dev), c.moves[b])
    same(gogame.batch_hash(c.states.copy()), c.hashes)     # the batch forms on arrays
    same(gogame.batch_move_hashes(c.states.copy()), c.moves)
    assert int(gogame.position_hash(np.zeros((6, N, N)))) == 0


@pytest.mark.parametrize('N', pc.SIZES)
def test_sub_batches_between_sentinels(N):
    """A lone board and a wave that is not full, from three places of the batch, written through out= into a slice of a larger
    int64 buffer 1, 2 or 3 words into it: nothing before or behind the slice is written.  The byte planes of the sub-batch
    start at an odd byte."""
    import torch
    from gymgo_amd import gogame
    P, A = N * N, N * N + 1
    for kind in SETS:
        c = he.case(N, kind)
        st = mc.to_dev(c.states.copy())
        tracked = gogame.batch_track(st)
        for nb in (1, 3):
            for k, first in enumerate((0, 7, B - nb)):
                lead, sl, n = k + 1, slice(first, first + nb), nb * A
                tag = (N, kind, nb, first)
                raw = torch.full((lead + n + 5,), SENTINEL, dtype=torch.int64, device='cuda')
                out = raw[lead:lead + n].view(nb, A)
                if k % 2 == 0:
                    buf = torch.zeros(1 + nb * 6 * P + 16, dtype=torch.uint8, device='cuda')
                    x = buf[1:1 + nb * 6 * P].view(nb, 6, N, N)
                    x.copy_(st[sl])
                    assert x.data_ptr() % 2 == 1
                    assert gogame.batch_move_hashes(x, out=out) is out
                    same(gogame.batch_hash(x), c.hashes[sl], tag)
                else:
                    assert gogame.batch_move_hashes_tracked(tracked[sl], out=out) is out
                    same(gogame.batch_hash_tracked(tracked[sl]), c.hashes[sl], tag)
                same(out, c.moves[sl], tag)
                assert bool((raw[:lead] == SENTINEL).all()) and bool((raw[lead + n:] == SENTINEL).all()), tag


@pytest.mark.parametrize('N', [n for n in fc.SIZES if n >= 3])
def test_flood_capture_boards(N):
    """The board-filling snake captured at the forced point: the longest flood and the longest XOR reduction."""
    from gymgo_amd import gogame
    from oracle import c_oracle
    c = fc.cases(N)
    idx = [i for i, k in enumerate(c.kind) if k == 'capture']
    assert idx
    states, q = c.states[idx], c.q[idx]
    want = he.batch_move_hashes(states)
    nxt, status = c_oracle.batch_next_states(states, q)
    assert not status.any()
    st = mc.to_dev(states.copy())
    for name, got in (('bytes', gogame.batch_move_hashes(st)), ('tracked', gogame.batch_move_hashes_tracked(gogame.batch_track(st)))):
        same(got, want, (N, name))
        got = mc.to_np(got)
        for i, a in enumerate(q):
            assert got[i, a] == he.hash_stones(nxt[i, 0], nxt[i, 1]) != got[i, N * N], (N, name, i)
    same(gogame.batch_hash(mc.to_dev(nxt)), want[np.arange(len(q)), q], (N, 'the hash of the child'))


H = 9
COUNTS = (0, 1, H, H + 5, -1)


def mask_case(N, kind):
    """Per board a history of H = 9 entries: [child 0, the parent's own hash, child 1, child 2, decoys ...] - the children of
    up to three candidates, a capturing one first where the board has one - and a count from COUNTS by the board's index."""
    c = he.case(N, kind)
    raw = oe.case(N, kind).raw
    hist = np.zeros((B, H), np.int64)
    count = np.array([COUNTS[b % len(COUNTS)] for b in range(B)], np.int32)
    chosen = 0
    for b, s in enumerate(c.states):
        cand = np.flatnonzero(oe.candidates(s).reshape(-1))
        caps = [a for a in cand if raw[b, 1].reshape(-1)[a] > 0]
        pick = (caps[:1] + [a for a in cand if a not in caps[:1]])[:3]
        entries = [int(c.moves[b, a]) for a in pick]
        chosen += len(pick)
        decoy = lambda i: he.signed((0x1234567 * (b + 1) + 0x9E3779B97F4A7C15 * (i + 1)) & he.MASK)
        row = [entries[0] if entries else decoy(0), int(c.hashes[b])] + [entries[i] if i < len(entries) else decoy(i) for i in (1, 2)]
        hist[b] = row + [decoy(i) for i in range(4, 4 + H - len(row))]
    return c, hist, count, chosen


@pytest.mark.parametrize('N', pc.SIZES)
def test_masks(N):
    import torch
    from gymgo_amd import gogame
    P = N * N
    total = 0
    for kind in SETS:
        c, hist, count, chosen = mask_case(N, kind)
        want = he.batch_repeat(c.states, c.moves, hist, count)
        full = he.batch_repeat(c.states, c.moves, hist, np.full(B, H, np.int32))
        cand = oe.candidates_of(c.states).reshape(B, P)
        assert not want[:, P].any() and not want[:, :P][~cand].any()              # the pass and non-candidates: never
        assert (full.sum(axis=1) >= want.sum(axis=1)).all()
        if chosen:
            assert full.sum() > want.sum() > 0 or N == 2, (N, kind)               # entries beyond count are ignored, and matter
        total += int(want.sum())
        st = mc.to_dev(c.states.copy())
        tracked = gogame.batch_track(st)
        history = history_of(hist, count)
        got = gogame.batch_superko_moves(st, history)
        assert got.dtype == torch.uint8
        same(got, want, (N, kind, 'bytes'))
        same(gogame.batch_superko_moves_tracked(tracked, history), want, (N, kind, 'tracked'))
        same(gogame.batch_superko_moves(st, history_of(hist, np.full(B, H, np.int32))), full, (N, kind, 'count = H'))
        same(gogame.batch_superko_moves(c.states.copy(), history), want, (N, kind, 'arrays'))
        # the parent's hash flags nothing by itself
        own = history_of(np.repeat(c.hashes[:, None], H, 1), np.full(B, H, np.int32))
        assert not he.batch_repeat(c.states, c.moves, np.repeat(c.hashes[:, None], H, 1), np.full(B, H)).any()
        assert not bool(gogame.batch_superko_moves(st, own).any()) and not bool(gogame.batch_superko_moves_tracked(tracked, own).any())
        # in place: plane 3 and the invalid rows keep what they had
        before = c.states[:, 3].copy()
        st2 = st.clone()
        assert gogame.batch_forbid_repeats(st2, history) is st2
        after = mc.to_np(st2)
        assert np.array_equal(after[:, 3], before | want[:, :P].reshape(B, N, N))
        assert np.array_equal(np.delete(after, 3, axis=1), np.delete(c.states, 3, axis=1))
        arr = c.states.copy()
        assert gogame.batch_forbid_repeats(arr, history) is arr and np.array_equal(arr, after)
        t0 = mc.to_np(tracked).copy()
        t2 = tracked.clone()
        assert gogame.batch_forbid_repeats_tracked(t2, history) is t2
        t1 = mc.to_np(t2)
        assert np.array_equal(t1[:, 2 * N:3 * N], t0[:, 2 * N:3 * N] | he.rows_of(want, N)), (N, kind)
        assert np.array_equal(np.delete(t1, np.s_[2 * N:3 * N], axis=1), np.delete(t0, np.s_[2 * N:3 * N], axis=1))
        same(gogame.batch_untrack(t2)[:, 3], after[:, 3], (N, kind, 'the tracked rows are plane 3'))
    assert total > 0, N


@pytest.mark.parametrize('N', (2, 3))
def test_real_games(N):
    """All (game, ply) pairs of the game set in one launch; then the games replayed with the repeats forbidden."""
    import torch
    from gymgo_amd import gogame
    g = he.games(N)
    states, hist, count = he.game_histories(g)
    assert states.shape[0] == 2560 and hist.shape == (2560, 41) and count.max() == 40
    want = he.batch_repeat(states, he.batch_move_hashes(states), hist, count)
    assert want.any()
    st = mc.to_dev(states.copy())
    history = history_of(hist, count)
    same(gogame.batch_superko_moves(st, history), want, (N, 'bytes'))
    same(gogame.batch_superko_moves_tracked(gogame.batch_track(st), history), want, (N, 'tracked'))
    # the replay: uniform among the points plane 3 allows after batch_forbid_repeats, the pass only when there is none
    G, T, P = he.GAMES, he.PLIES, N * N
    rs = np.random.RandomState(he.GAME_SEEDS[N])
    cur = torch.zeros((G, 6, N, N), dtype=torch.uint8, device='cuda')
    seen = gogame.PositionHistory(G, T + 1).push(gogame.batch_hash(cur))
    keys = [{he.position_key(np.zeros((N, N)), np.zeros((N, N)))} for _ in range(G)]
    forbidden = board_moves = 0
    for t in range(T):
        free0 = mc.to_np(cur[:, 3]).reshape(G, P) == 0
        gogame.batch_forbid_repeats(cur, seen)
        host = mc.to_np(cur)
        live = np.flatnonzero(host[:, 5, 0, 0] == 0)
        if not len(live):
            break
        free = host[:, 3].reshape(G, P) == 0
        forbidden += int((free0 & ~free)[live].sum())
        acts = np.array([int(np.flatnonzero(free[b])[rs.randint(free[b].sum())]) if free[b].any() else P for b in live], np.int32)
        idx = torch.from_numpy(live).cuda()
        nxt, status = gogame.batch_next_states(cur[idx], torch.from_numpy(acts).cuda(), check=False)
        assert not bool(status.any())
        cur[idx] = nxt
        mask = torch.zeros(G, dtype=torch.bool, device='cuda')
        mask[idx] = True
        seen.push(gogame.batch_hash(cur), mask)
        after = mc.to_np(nxt)
        for b, a, s in zip(live, acts, after):
            k = he.position_key(s[0], s[1])
            if a < P:
                board_moves += 1
                assert k not in keys[b], (N, t, b, a)          # never a position the game has been in
            keys[b].add(k)
    assert forbidden > 0 and board_moves > 0, (N, forbidden, board_moves)
    assert mc.to_np(seen.count).max() <= T + 1


def test_empty_batch_and_argument_errors():
    import torch
    from gymgo_amd import gogame
    from gymgo_amd._lib import GymGoNativeError
    for N in (2, 9, 13, 19):
        A = N * N + 1
        empty = torch.empty((0, 6, N, N), dtype=torch.uint8, device='cuda')
        tracked = torch.empty((0, 5 * N + 1), dtype=torch.int32, device='cuda')
        none = gogame.PositionHistory(0, 4)
        assert tuple(gogame.batch_hash(empty).shape) == (0,) == tuple(gogame.batch_hash_tracked(tracked).shape)
        assert tuple(gogame.batch_move_hashes(empty).shape) == (0, A) == tuple(gogame.batch_move_hashes_tracked(tracked).shape)
        assert tuple(gogame.batch_superko_moves(empty, none).shape) == (0, A) == tuple(gogame.batch_superko_moves_tracked(tracked, none).shape)
        assert gogame.batch_forbid_repeats(empty, none) is empty and gogame.batch_forbid_repeats_tracked(tracked, none) is tracked
    N, A = 5, 26
    st = mc.to_dev(he.case(N, 'policy').states[:2].copy())
    tracked = gogame.batch_track(st)
    hist = gogame.PositionHistory(2, 3)
    assert hist.hashes.is_cuda and hist.count.is_cuda
    for fn, x in ((gogame.batch_hash, st), (gogame.batch_move_hashes, st), (gogame.batch_hash_tracked, tracked),
                  (gogame.batch_move_hashes_tracked, tracked)):
        with pytest.raises(GymGoNativeError):
            fn(x.cpu())                                                        # a host tensor never computes
    with pytest.raises(GymGoNativeError):
        gogame.batch_superko_moves(st.cpu(), hist)
    with pytest.raises(GymGoNativeError):
        gogame.batch_superko_moves(st, gogame.PositionHistory(2, 3, device='cpu'))
    for bad in ((hist.hashes.to(torch.int32), hist.count), (hist.hashes, hist.count.to(torch.int64)), (hist.hashes[:1], hist.count),
                (hist.hashes, hist.count[:1]), (hist.hashes.t(), hist.count), None):
        for fn, x in ((gogame.batch_superko_moves, st), (gogame.batch_superko_moves_tracked, tracked),
                      (gogame.batch_forbid_repeats, st), (gogame.batch_forbid_repeats_tracked, tracked)):
            with pytest.raises(ValueError):
                fn(x, bad)
    for out in (torch.empty((2, A), dtype=torch.int32, device='cuda'), torch.empty((1, A), dtype=torch.int64, device='cuda'),
                torch.empty((2, A + 1), dtype=torch.int64, device='cuda'), torch.empty((2, A), dtype=torch.int64),
                torch.empty((2, 2 * A), dtype=torch.int64, device='cuda')[:, ::2]):
        with pytest.raises(ValueError):
            gogame.batch_move_hashes(st, out=out)
        with pytest.raises(ValueError):
            gogame.batch_move_hashes_tracked(tracked, out=out)


# ---------------------------------------------------------------- the search
def roots7(N, seed=60):
    """7 roots of size 2 or 3 (the crafted roots of the other search tests need N >= 4): the empty board, five positions after
    1 .. 5 plies of random play, a finished game."""
    roots = mc.make_roots(N, 7, seed + N, max_ply=N * N, step=1)
    assert roots.shape[0] == 7 and not roots[0, :2].any() and roots[-1, 5, 0, 0] == 1 and (roots[:-1, 5, 0, 0] == 0).all()
    return roots


def recreations(states, actions, final):
    """The (game, move) pairs of recorded games (states [R, M, 6, N, N] before each move, actions [R, M], final [R, 6, N, N])
    where a board move made a position, compared stone by stone, that the game had been in before."""
    R, M = actions.shape
    P = states.shape[-1] ** 2
    out = []
    for r in range(R):
        keys = set()
        for t in range(M):
            keys.add(he.position_key(states[r, t, 0], states[r, t, 1]))
            nxt = states[r, t + 1] if t + 1 < M else final[r]
            if 0 <= actions[r, t] < P and he.position_key(nxt[0], nxt[1]) in keys:
                out.append((r, t))
    return out


def test_search_forbids_repeats_at_the_roots():
    import torch
    from gymgo_amd import gogame
    N, R, P = 3, 7, 9
    roots = roots7(N)
    st = mc.to_dev(roots)
    E = tsio.on_device(tsio.point_evaluator)
    search = gogame.PuctSearch(st, 8, c=0.6, komi=0.5, leaves=2, features=torch.float16)
    for _ in range(4):
        search.backup(*E(*search.select()))
    legal0 = mc.to_np(search.result().legal).copy()
    visits0 = mc.to_np(search.result().visits).copy()
    moves = he.batch_move_hashes(roots)
    hist, count = np.zeros((R, 2), np.int64), np.zeros(R, np.int32)
    for r in range(R):
        pick = np.flatnonzero(legal0[r, :P])[:2]           # the children of the first two legal points
        hist[r, :len(pick)], count[r] = moves[r, pick], len(pick)
    history = history_of(hist, count)
    rep = he.batch_repeat(roots, moves, hist, count).astype(bool)
    assert rep.any() and (visits0[rep] > 0).any()           # some forbidden action has a child with visits already
    same(gogame.batch_superko_moves(st, history), rep.astype(np.uint8))
    pending = search.select()
    with pytest.raises(ValueError):
        search.forbid_repeats(history)                       # leaves are pending
    search.backup(*E(*pending))
    search.forbid_repeats(history)
    assert np.array_equal(mc.to_np(search.result().legal), legal0 & ~rep)
    for _ in range(3):
        search.backup(*E(*search.select()))
    acts, pi, value = search.root_policy()
    assert not mc.to_np(pi)[rep].any()                       # no visits counted under a forbidden action
    acts = mc.to_np(acts)
    assert not rep[np.arange(R)[acts >= 0], acts[acts >= 0]].any()
    with pytest.raises(ValueError):
        search.forbid_repeats(gogame.PositionHistory(R + 1, 2))


@pytest.mark.parametrize('N', (2, 3))
def test_selfplay_with_superko_never_recreates_a_position(N):
    import torch
    from gymgo_amd import gogame
    M, T = 24, 4
    # (the roots of seed 60 play 24 moves at 3x3 without a repetition, with the rule or without: measured on the device, these
    # roots repeat a position 15 times at 2x2 and once at 3x3 - the game of root 5, which the rule makes 7 moves longer)
    st = mc.to_dev(roots7(N, seed=90))
    E = tsio.on_device(tsio.point_evaluator)
    kw = dict(c=0.6, komi=0.5, leaves=2, capacity=512, features=torch.float16, record_states=True, seed=7)
    on = gogame.puct_selfplay(st, M, T, E, superko=True, **kw)
    off = gogame.puct_selfplay(st, M, T, E, superko=False, **kw)
    plain = gogame.puct_selfplay(st, M, T, E, **kw)
    tgf.same_tuples(off, plain, N)                           # superko=False: bit for bit today's records
    host = lambda rec: (mc.to_np(rec.states), mc.to_np(rec.actions), mc.to_np(rec.final_states))
    assert recreations(*host(off)), N                        # the premise: without the rule some game repeats a position
    assert not recreations(*host(on)), N


def test_puct_play_superko_keyword():
    import torch
    from gymgo_amd import gogame
    N, M, T = 3, 6, 4
    st = mc.to_dev(roots7(N))
    E = tsio.on_device(tsio.point_evaluator)
    kw = dict(c=0.6, komi=0.5, leaves=2, capacity=128, features=torch.float16)
    for reuse in (True, False):
        a = gogame.puct_play(st, M, T, E, reuse=reuse, superko=False, **kw)
        b = gogame.puct_play(st, M, T, E, reuse=reuse, **kw)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), reuse
        acts, final = gogame.puct_play(st, M, T, E, reuse=reuse, superko=True, **kw)
        assert tuple(acts.shape) == (7, M) and tuple(final.shape) == (7, 6, N, N)
        # replayed on the host: no board move recreates an earlier position of its game
        from oracle import c_oracle
        cur, acts = roots7(N).copy(), mc.to_np(acts)
        keys = [{he.position_key(s[0], s[1])} for s in cur]
        for t in range(M):
            for r in np.flatnonzero(acts[:, t] >= 0):
                s = cur[r].copy()
                s[3] = 0
                nxt, status = c_oracle.batch_next_states(s[None], acts[r:r + 1, t].astype(np.int32))
                assert not status[0]
                k = he.position_key(nxt[0, 0], nxt[0, 1])
                assert acts[r, t] == N * N or k not in keys[r], (reuse, r, t)
                keys[r].add(k)
                cur[r] = nxt[0]
        assert np.array_equal(cur[:, :2], mc.to_np(final)[:, :2])
