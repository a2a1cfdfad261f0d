"""The premises of tests/flood_cases.py, on the CPU: the crafted boards are what their kinds say, at every board size, and the
launches of tests/test_gpu_flood_sizes.py do play the forced points.  A plain group walker (flood_cases.group) and the C oracle."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import flood_cases as fc

SIZES = list(fc.SIZES)


def _rows(N, *kinds):
    c = fc.cases(N)
    return [(i, c.states[i], tuple(int(v) for v in divmod(int(c.point[i]), N)), tuple(int(v) for v in c.seed[i]), int(c.variant[i]))
            for i in range(len(c.kind)) if c.kind[i] in kinds]


def _after(N, s, q):
    from oracle import c_oracle
    nxt, status = c_oracle.batch_next_states(s[None], np.array([q[0] * N + q[1]], np.int32))
    return nxt[0], int(status[0])


@pytest.mark.parametrize('N', SIZES)
def test_every_kind_is_there_in_every_orientation_and_every_group_has_a_liberty(N):
    c = fc.cases(N)
    count = {k: c.kind.count(k) for k in fc.KINDS}
    assert count['shape'] == 24
    if N >= 5:
        for kind in fc.TURNED:
            assert sorted(c.variant[[i for i, k in enumerate(c.kind) if k == kind]].tolist()) == list(range(16)), kind
    if N >= 3:
        assert count['capture'] > 0 and count['corridor'] == count['capture']
    assert len(c.kind) <= 128
    for i, s in enumerate(c.states):
        assert fc.every_group_has_a_liberty(s), (N, i, c.kind[i])
        assert not (s[0] & s[1]).any() and s.max() <= 1
        occupied = (s[0] | s[1]) == 1
        assert (s[3][occupied] == 1).all(), (N, i)
        for plane in (2, 4, 5):
            assert s[plane].min() == s[plane].max()
        if c.kind[i] in fc.FORCED:       # forced: the draw can take q or the pass
            assert c.q[i] == c.point[i] >= 0 and s[3].sum() == N * N - 1 and s[3].reshape(-1)[c.q[i]] == 0
        else:
            assert c.q[i] == -1
    b = fc.batch(N)
    assert b.states.shape == (fc.BATCH, 6, N, N) and all(k == 'random' for k in b.kind[3::4])
    assert set(b.index[b.index >= 0].tolist()) == set(range(len(c.kind)))         # every crafted board is in the batch


@pytest.mark.parametrize('N', SIZES[1:])
def test_the_group_under_test_has_the_liberties_of_its_kind_and_q_does_what_the_kind_says(N):
    for i, s, q, seed, v in _rows(N, 'capture', 'atari'):
        mover = int(s[2, 0, 0])
        stones, libs = fc.group(s, seed)
        assert s[1 - mover][seed] and seed in fc.neighbours(q, N)
        kind = fc.cases(N).kind[i]
        assert len(libs) == (1 if kind == 'capture' else 2) and q in libs, (N, i, libs)
        nxt, status = _after(N, s, q)
        assert status == 0
        want = s[:2].copy()
        want[mover][q] = 1
        if kind == 'capture':            # exactly the snake leaves the board, nothing else changes
            for p in stones:
                want[1 - mover][p] = 0
            if N >= 5:
                assert len(stones) >= (N - 2) ** 2 / 2 - N, (N, len(stones))
        assert np.array_equal(nxt[:2], want), (N, i)
        if kind == 'atari':              # one liberty left, at the far end of the flood, and the mover may take it later
            far = fc.group(nxt, seed)[1]
            assert len(far) == 1 and fc.group(nxt, seed)[0] == stones
            back, status = _after(N, nxt, (N, 0))          # the snake's side passes: the mover may take that liberty
            assert status == 0 and back[3][next(iter(far))] == 0
            if N >= 5:
                steps = fc.vertical_steps({(c, r) for r, c in stones}, seed[::-1]) if v & 1 else fc.vertical_steps(stones, seed)
                end = [p for p in fc.neighbours(next(iter(far)), N) if p in stones]
                assert [steps[p[::-1] if v & 1 else p] for p in end] == [max(steps.values())], (N, i)
    for i, s, q, seed, v in _rows(N, 'join1', 'join2'):
        mover = int(s[2, 0, 0])
        kind = fc.cases(N).kind[i]
        mine = [p for p in fc.neighbours(q, N) if s[mover][p]]
        groups = {frozenset(fc.group(s, p)[0]) for p in mine}
        assert len(groups) == 2 and seed == q, (N, i)                   # q touches the snake and a second group of the mover
        assert any(fc.group(s, p)[1] == {q} for p in mine)              # ... and is the last liberty of one of them
        nxt, status = _after(N, s, q)
        assert status == 0
        want = s[:2].copy()
        want[mover][q] = 1
        assert np.array_equal(nxt[:2], want), (N, i)                     # nothing is captured
        stones, libs = fc.group(nxt, q)
        assert stones == set().union(*groups) | {q} and len(libs) == (1 if kind == 'join1' else 2), (N, i, libs)
        assert all(nxt[3][p] == 0 for p in libs) or kind == 'join2'      # the opponent may capture the joined group
    for i, s, q, seed, v in _rows(N, 'suicide'):
        mover = int(s[2, 0, 0])
        assert s[mover][seed] and fc.group(s, seed)[1] == {q}
        assert s[3][q] == 1 and not s[0][q] and not s[1][q]
        assert np.array_equal(s[3], fc.invalid_moves(s))
        assert _after(N, s, q)[1] != 0


@pytest.mark.parametrize('N', SIZES[3:])
def test_the_flood_is_as_deep_as_the_board_allows(N):
    """Depth: the fewest vertical steps on a path inside the group from its seed to its farthest stone.  Unturned (and flipped)
    boards hold it in vertical steps, boards a quarter turn on in horizontal ones."""
    bound = N - 1 if N < 9 else 2 * N
    seen = set()
    for i, s, q, seed, v in _rows(N, 'capture', 'atari', 'join1', 'join2', 'suicide'):
        kind = fc.cases(N).kind[i]
        if kind in ('join1', 'join2'):
            s = _after(N, s, q)[0]
        stones = fc.group(s, seed)[0]
        quarter = (v & 7) & 1
        if quarter:
            stones, seed = {(c, r) for r, c in stones}, (seed[1], seed[0])        # horizontal steps of the board as it is
        d = fc.vertical_depth(stones, seed)
        assert d >= (bound - 1 if kind == 'suicide' else bound), (N, kind, v, d)    # (the suicide snake lacks the stone at q)
        seen.add((kind, quarter))
    assert len(seen) == 10
    # the region the capture leaves is as deep, and it is empty: flood it as if it were stones
    for i, s, q, seed, v in _rows(N, 'corridor'):
        e = np.zeros_like(s)
        e[0] = (s[0] | s[1]) == 0
        region = fc.group(e, seed)[0]
        assert len(region) >= (N - 2) ** 2 / 2 - N
        if v & 1:
            region, seed = {(c, r) for r, c in region}, seed[::-1]
        assert fc.vertical_depth(region, seed) >= bound, (N, v)


@pytest.mark.parametrize('N', SIZES)
def test_the_oracle_takes_the_forced_point_on_the_first_ply_in_every_rollout_cell(N):
    """Coverage, a condition: for every batch size the GPU test launches a rollout at (board b always draws from generator
    (SEED, b)), at least a quarter of the forced boards of each kind take q on ply 1 - and each kind is there."""
    b = fc.batch(N)
    kinds_here = {k for k in fc.cases(N).kind if k in fc.FORCED}
    if N >= 5:
        assert kinds_here == set(fc.FORCED)
    for B in fc.rollout_batches(N):
        last = fc.first_ply(N, B)
        for kind in kinds_here:
            on = [i for i in range(B) if b.kind[i] == kind]
            hit = [i for i in on if last[i] == b.q[i]]
            assert on and 4 * len(hit) >= len(on), (N, B, kind, len(hit), len(on))
        for i in range(B):
            if b.kind[i] in fc.FORCED:
                assert last[i] in (b.q[i], N * N), (N, B, i)
            if b.kind[i] == 'suicide':
                assert last[i] != fc.cases(N).point[b.index[i]], (N, B, i)
