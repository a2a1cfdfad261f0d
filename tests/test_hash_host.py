"""CPU: what tests/test_gpu_hash.py relies on, without a device.  The key table; the expectation of the move hashes
(tests/hash_expect.py) against the positions the C restatement plays; the capture classes the sets hold; the board-filling
snake of tests/flood_cases.py, the longest XOR reduction there is; the game set on which positions repeat; PositionHistory
against a NumPy ring; the argument checks that need no device."""
import numpy as np
import pytest

import flood_cases as fc
import hash_expect as he
import outcome_expect as oe
import plane_cases as pc

SETS = ('policy', 'clean')
HOST_SIZES = (2, 3, 5, 9, 13, 19)


def test_keys():
    from gymgo_amd import gogame
    assert len(he.KEYS) == 722 == len(set(he.KEYS)) and all(0 < k < 2 ** 64 for k in he.KEYS)
    assert he.key(0, 0, 0) == 0xc8a43d929c6a465e and he.key(1, 18, 18) == 0x345c2fd1bcdda841
    keys = gogame.zobrist_keys()
    assert isinstance(keys, np.ndarray) and keys.dtype == np.int64 and keys.shape == (2, 19, 19)
    assert keys.view(np.uint64).reshape(-1).tolist() == he.KEYS
    assert gogame.HASH_SEED == he.SEED
    assert he.hash_of(np.zeros((6, 7, 7), np.uint8)) == 0
    # all 3^9 positions of a 3x3 corner hash differently
    seen = set()
    for code in range(3 ** 9):
        h = 0
        for i in range(9):
            v = code // 3 ** i % 3
            if v:
                h ^= he.key(v - 1, i // 3, i % 3)
        seen.add(h)
    assert len(seen) == 3 ** 9


@pytest.mark.parametrize('N', HOST_SIZES)
def test_move_hashes_agree_with_the_positions_the_restatement_plays(N):
    from oracle import c_oracle
    by_hash, suicides = {}, {}
    for kind in SETS:
        c = he.case(N, kind)
        raw = oe.case(N, kind).raw
        cand = oe.candidates_of(c.states)
        where = np.argwhere(cand)
        suicides[kind] = 0
        assert np.array_equal(c.hashes, c.moves[:, N * N])                      # the pass
        flat = cand.reshape(len(cand), -1)
        assert (c.moves[:, :N * N][~flat] == np.repeat(c.hashes[:, None], N * N, 1)[~flat]).all()   # non-candidates
        if not len(where):
            continue
        acts = (where[:, 1] * N + where[:, 2]).astype(np.int32)
        played = c.states[where[:, 0]].copy()
        played[:, 3] = 0                                                      # (the restatement refuses a point of plane 3)
        nxt, status = c_oracle.batch_next_states(played, acts)
        for (b, y, x), a, child, bad in zip(where, acts, nxt, status):
            if raw[b, 0, y, x] == 0:      # a suicide (clean boards only): no position of the game; the hash keeps the stone
                suicides[kind] += 1
                bl, wh, _, _ = he.child(c.states[b], y, x)
                assert c.moves[b, a] == he.hash_stones(bl, wh)
                continue
            assert not bad, (N, kind, b, y, x)
            assert c.moves[b, a] == he.hash_stones(child[0], child[1]), (N, kind, b, y, x)
            key = he.position_key(child[0], child[1])
            assert by_hash.setdefault(int(c.moves[b, a]), key) == key, (N, kind, b, y, x)   # distinct positions, distinct hashes
    assert suicides['policy'] == 0
    assert len(by_hash) > 1 or N == 2


# the capture classes of the candidates, over both sets: (captures >= 2 stones, captures >= 2 separate chains, has a
# one-liberty opponent neighbour).  The sizes where a class is empty are named here: no candidate of the 42 boards captures
# two separate chains at 2x2 and at 3x3.
EMPTY_CLASSES = {2: (False, True, False), 3: (False, True, False)}


@pytest.mark.parametrize('N', HOST_SIZES)
def test_the_sets_hold_the_capture_classes(N):
    stones2 = chains2 = atari = 0
    for kind in SETS:
        c = he.case(N, kind)
        for b, s in enumerate(c.states):
            for y, x in np.argwhere(oe.candidates(s)):
                _, _, n, chains = he.child(s, int(y), int(x))
                stones2 += n >= 2
                chains2 += chains >= 2
                atari += n >= 1
    empty = EMPTY_CLASSES.get(N, (False, False, False))
    assert (stones2 == 0, chains2 == 0, atari == 0) == empty, (N, stones2, chains2, atari)


@pytest.mark.parametrize('N', fc.SIZES)
def test_the_snake_is_captured_at_the_forced_point(N):
    from oracle import c_oracle
    c = fc.cases(N)
    idx = [i for i, k in enumerate(c.kind) if k == 'capture']
    if N < 3:
        assert not idx          # no room for a snake
        return
    assert idx, N
    states, q = c.states[idx], c.q[idx]
    nxt, status = c_oracle.batch_next_states(states, q)
    assert not status.any()
    for s, a, child, seed in zip(states, q, nxt, c.seed[idx]):
        moves = he.move_hashes(s)
        assert moves[a] == he.hash_stones(child[0], child[1])
        snake, _ = fc.group(s, tuple(int(v) for v in seed))
        _, _, n, chains = he.child(s, a // N, a % N)
        assert n == len(snake) and chains == 1
        assert (np.delete(moves, a) == he.hash_of(s)).all()      # forced: q is the only candidate
    if N >= 5:
        assert n == len(fc.snake(N)[0])


def test_positions_repeat_in_the_game_set():
    counts = {}
    for N in (2, 3):
        g = he.games(N)
        assert g.states.shape == (he.GAMES, he.PLIES, 6, N, N) == (64, 40, 6, N, N)
        counts[N] = sum(1 for game in g.states if he.recreating_moves(game))
    print('games with a move that recreates a position:', counts)
    assert counts[2] >= 32 and counts[3] >= 8, counts


def test_position_history_is_a_ring():
    import torch
    from gymgo_amd import gogame
    B, H = 5, 4
    hist = gogame.PositionHistory(B, H, device='cpu')
    assert hist.hashes.dtype == torch.int64 and tuple(hist.hashes.shape) == (B, H) and not hist.hashes.any()
    assert hist.count.dtype == torch.int32 and tuple(hist.count.shape) == (B,) and hist.capacity == H
    model, count = np.zeros((B, H), np.int64), np.zeros(B, np.int32)
    rs = np.random.RandomState(3)
    for step in range(3 * H + 2):
        h = rs.randint(-2 ** 62, 2 ** 62, size=B).astype(np.int64)
        mask = None if step % 3 == 0 else rs.randint(0, 2, size=B).astype(bool)
        arg = None if mask is None else (torch.from_numpy(mask) if step % 3 == 1 else torch.from_numpy(mask.astype(np.uint8)))
        assert hist.push(torch.from_numpy(h), arg) is hist
        sel = np.ones(B, bool) if mask is None else mask
        for b in np.flatnonzero(sel):
            model[b, count[b] % H] = h[b]
            count[b] += 1
        assert np.array_equal(hist.hashes.numpy(), model) and np.array_equal(hist.count.numpy(), count), step
        if step == 2 * H:
            m = np.array([1, 0, 0, 1, 0], bool)
            assert hist.reset(torch.from_numpy(m)) is hist
            model[m], count[m] = 0, 0
            assert np.array_equal(hist.hashes.numpy(), model) and np.array_equal(hist.count.numpy(), count)
    assert count.max() > H                     # past capacity: the last H positions
    hist.reset()
    assert not hist.hashes.any() and not hist.count.any()
    for bad in (lambda: gogame.PositionHistory(2, 0, device='cpu'), lambda: gogame.PositionHistory(-1, 3, device='cpu'),
                lambda: hist.push(torch.zeros(B, dtype=torch.int32)), lambda: hist.push(torch.zeros(B + 1, dtype=torch.int64)),
                lambda: hist.push(torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64)),
                lambda: hist.reset(torch.zeros(B - 1, dtype=torch.bool))):
        with pytest.raises(ValueError):
            bad()


def test_entry_point_argument_checks_without_device(native_built):
    """The checks of the four entry points in the header's order, before any device work.  No call here passes them all."""
    from gymgo_amd import _lib
    L = _lib.lib()
    p, odd = 4096, 4100          # stand-ins for device pointers: never dereferenced by a call that fails a check
    for fn in (L.gg_batch_hash, L.gg_batch_hash_tracked):
        assert fn(p, p, 2, 1, None) == -1 and fn(p, p, 2, 20, None) == -1 and fn(p, p, -1, 9, None) == -1
        assert fn(None, None, 0, 9, None) == 0
        assert fn(None, p, 2, 9, None) == -2 and fn(p, None, 2, 9, None) == -2
        assert fn(p, odd, 2, 9, None) == -3
    for fn in (L.gg_batch_move_hashes, L.gg_batch_move_hashes_tracked):
        assert fn(p, p, p, 4, p, p, p, 2, 1, None) == -1 and fn(p, p, p, 4, p, p, p, 2, 20, None) == -1
        assert fn(p, p, p, 4, p, p, p, -1, 9, None) == -1
        assert fn(p, p, p, -1, p, p, p, 2, 9, None) == -3            # H
        assert fn(p, p, p, -1, p, p, p, 2, 0, None) == -1            # ... after the size
        assert fn(None, None, None, 0, None, None, None, 0, 9, None) == 0
        assert fn(None, None, None, -1, None, None, None, 0, 9, None) == -3   # ... before the empty batch
        assert fn(None, p, p, 4, p, p, p, 2, 9, None) == -2
        assert fn(p, p, p, 4, None, None, None, 2, 9, None) == -2    # no output
        assert fn(p, None, p, 4, None, p, None, 2, 9, None) == -2    # repeat needs the history
        assert fn(p, p, None, 4, None, None, p, 2, 9, None) == -2    # rows need the count
        assert fn(p, None, None, 0, None, p, None, 2, 9, None) == -2
        assert fn(p, None, None, 0, odd, None, None, 2, 9, None) == -3
        assert fn(p, p, p, 4, None, None, odd + 2, 2, 9, None) == -3
        assert fn(p, odd, p, 4, None, p, None, 2, 9, None) == -3
        assert fn(p, p, odd + 2, 4, None, p, None, 2, 9, None) == -3


def test_wrapper_argument_checks_without_device():
    """Shapes and dtypes raise ValueError before a device is touched."""
    import torch
    from gymgo_amd import gogame
    st = np.zeros((2, 6, 5, 5), np.uint8)
    tracked = torch.zeros((2, 26), dtype=torch.int32)
    hist = gogame.PositionHistory(2, 3, device='cpu')
    wrong = [gogame.PositionHistory(3, 3, device='cpu'), (hist.hashes.to(torch.int32), hist.count), (hist.hashes, hist.count.long()),
             (hist.hashes[:, 0], hist.count), (hist.hashes.numpy(), hist.count.numpy()), None, object()]
    for fn, x in ((gogame.batch_superko_moves, st), (gogame.batch_forbid_repeats, st), (gogame.batch_superko_moves_tracked, tracked),
                  (gogame.batch_forbid_repeats_tracked, tracked)):
        for h in wrong:
            with pytest.raises(ValueError):
                fn(x, h)
    for fn in (gogame.batch_hash, gogame.batch_move_hashes):
        with pytest.raises(ValueError):
            fn(np.zeros((2, 5, 5, 5), np.uint8))
        with pytest.raises(ValueError):
            fn(np.zeros((2, 6, 5, 4), np.uint8))
    for fn in (gogame.batch_hash_tracked, gogame.batch_move_hashes_tracked):
        with pytest.raises(ValueError):
            fn(torch.zeros((2, 27), dtype=torch.int32))
        with pytest.raises(ValueError):
            fn(torch.zeros((2, 26), dtype=torch.int64))
        with pytest.raises(ValueError):
            fn(np.zeros((2, 26), np.int32))
    for out in (torch.zeros((2, 26), dtype=torch.int32), torch.zeros((3, 26), dtype=torch.int64), np.zeros((2, 26), np.int64)):
        with pytest.raises(ValueError):
            gogame.batch_move_hashes(st, out=out)
        with pytest.raises(ValueError):
            gogame.batch_move_hashes_tracked(tracked, out=out)
    with pytest.raises(ValueError):
        gogame.batch_forbid_repeats(torch.zeros((2, 6, 5, 5), dtype=torch.float32), hist)
