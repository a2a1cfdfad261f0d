"""Positions that make a flood work as hard as the board allows, for EVERY board size from 2 to 19 - test infrastructure, CPU
only, NumPy (and the C oracle for the planes only it can fill).  tests/test_flood_cases_host.py asserts their premises,
tests/test_gpu_flood_sizes.py sends them through every step and rollout kernel.

The gadget is a one-stone-wide snake: legs on the columns 1, 3, 5, ... over the rows 1 .. N-2, joined alternately at the bottom
and at the top, inside a ring of the other colour that also holds the teeth between the legs.  A flood seeded at the free end
of the last leg reaches the free end of the first after (legs) x (N - 3) vertical steps: 144 at 19x19, 60 at 13x13, 28 at 10x10.
`q` is the point the board is about; the kinds:
  capture   the opponent's snake with q, the ring point beyond the free end of its last leg, as its only liberty; two corners
            that do not touch q are empty, so every group of the mover has a liberty.  q captures the whole snake.
  atari     the same with the ring point beyond the free end of the FIRST leg empty too: after q the snake has one liberty, at
            the far end of the flood from the stone next to q.
  join1     the colours swapped and the last leg one stone shorter: q is the point it left, the snake's last liberty, and
  join2     touches the mover's stone on the ring beyond it (a ring point in line with q cannot: its neighbours along the ring
            touch the snake or a tooth).  The joined group spans the board and has exactly one liberty / exactly two.
  suicide   as join without that stone (and with the two empty corners): q is suicide.  Plane 3 is the oracle's: q is marked.
  corridor  a capture board after the capture (the oracle's next state, its plane 3): a snake-shaped empty region.
  shape     tests/test_gpu_adversarial.consistent_boards(N): spirals, serpentines and combs, plane 3 from the oracle.
A capture, atari or join board is FORCED: plane 3 is 1 everywhere but at q, so a draw takes q or the pass.  Every forced kind,
suicide and corridor come in all eight orientations (a quarter turn makes the vertical depth runs of N - 2 stones for the
horizontal fill, the flips put the seed on either edge) and with either colour to move.  Below 5x5 the snake degenerates: what
is built there is kept if every group on it has a liberty and q does what its kind says, and is held to nothing else."""
import functools
from types import SimpleNamespace

import numpy as np

SIZES = tuple(range(2, 20))
FORCED = ('capture', 'atari', 'join1', 'join2')
TURNED = FORCED + ('suicide', 'corridor')          # sixteen variants each: eight orientations x the colour to move
KINDS = TURNED + ('shape',)
BATCH = 256
# The generators of tests/test_gpu_flood_sizes.py: board b of a launch of ANY batch size draws from generator (SEED, b), so the
# B boards of a cell are the first B of batch(N) with the first B of these generators.  Chosen so that the oracle takes q on
# the first ply on at least a quarter of the forced boards of each kind in every cell, at every N (a forced board draws between
# two actions whatever N is; test_flood_cases_host asserts the condition).
SEED = 6


def turn(a, k):
    """The k-th of the eight orientations on the last two axes: k & 3 quarter turns, then a flip if k & 4."""
    a = np.rot90(a, k & 3, axes=(-2, -1))
    return a[..., ::-1] if k & 4 else a


def turn_point(p, k, N):
    """where the point p = (row, column) of the unturned board lies on the turned one"""
    at = np.argwhere(turn(np.arange(N * N).reshape(N, N), k) == p[0] * N + p[1])[0]
    return int(at[0]), int(at[1])


def neighbours(p, N):
    return [(r, c) for r, c in ((p[0] - 1, p[1]), (p[0] + 1, p[1]), (p[0], p[1] - 1), (p[0], p[1] + 1)) if 0 <= r < N and 0 <= c < N]


def snake(N):
    """(stones, columns of the legs, row of the ring beyond the free end of the last leg)"""
    cols = list(range(1, N - 1, 2))
    pts = {(r, c) for c in cols for r in range(1, N - 1)}
    for i in range(len(cols) - 1):
        pts.add((N - 2 if i % 2 == 0 else 1, cols[i] + 1))
    r0 = 0 if len(cols) >= 2 and len(cols) % 2 == 0 else N - 1         # the last join is at the bottom: the free end is the top
    return pts, cols, r0


def _corners(N, q, count=2):
    """empty corners: not next to q, and never (0, 0), which touches the second liberty of the atari boards"""
    return [c for c in ((N - 1, 0), (N - 1, N - 1), (0, N - 1)) if c not in neighbours(q, N) and c != q][:count]


def _grid(N, kind):
    """-> (grid of 'X' mover / 'O' opponent / '.', q, seed) of the unturned board, or None where N has no room for it"""
    pts, cols, r0 = snake(N)
    if not cols:
        return None
    cl = cols[-1]
    r1 = 1 if r0 == 0 else N - 2
    if kind in ('capture', 'atari'):
        g = np.full((N, N), 'X')
        for p in pts:
            g[p] = 'O'
        q = (r0, cl)
        for p in [q] + _corners(N, q) + ([(0, 1)] if kind == 'atari' else []):
            g[p] = '.'
        return g, q, (r1, cl)
    q = (r1, cl)
    pts = pts - {q}
    if not pts:
        return None
    g = np.full((N, N), 'O')
    for p in pts:
        g[p] = 'X'
    g[q] = '.'
    if kind == 'suicide':
        for p in _corners(N, q):
            g[p] = '.'
        return g, q, (r1 + (1 if r0 == 0 else -1), cl)
    g[r0, cl] = 'X'
    g[r0, cl - 1] = '.'
    if kind == 'join2':
        g[r0, cl + 1] = '.'
    return g, q, q                 # the group under test is the one the stone at q makes


def _state(g, white_to_move):
    s = np.zeros((6,) + g.shape, np.uint8)
    s[1 if white_to_move else 0] = g == 'X'
    s[0 if white_to_move else 1] = g == 'O'
    s[2] = white_to_move
    return s


def group(s, p):
    """stones and liberties of the group at p, by a stack flood"""
    N = s.shape[-1]
    col = 0 if s[0][p] else 1
    assert s[col][p], p
    stones, libs, todo = {p}, set(), [p]
    while todo:
        for n in neighbours(todo.pop(), N):
            if s[col][n]:
                if n not in stones:
                    stones.add(n)
                    todo.append(n)
            elif not s[1 - col][n]:
                libs.add(n)
    return stones, libs


def every_group_has_a_liberty(s):
    seen = set()
    for plane in (0, 1):
        for p in map(tuple, np.argwhere(s[plane] == 1)):
            if p not in seen:
                stones, libs = group(s, p)
                if not libs:
                    return False
                seen |= stones
    return True


def invalid_moves(s):
    """the oracle's plane 3 for the side to move, no ko (its `player` is the side that moved last, as in next_state)"""
    from oracle import c_oracle
    return c_oracle.compute_invalid_moves(s, 1 - int(s[2, 0, 0]))


def _fits(s, kind, q, seed):
    """what a degenerate board (N < 5) must still do to be kept"""
    from oracle import c_oracle
    if not every_group_has_a_liberty(s):
        return False
    N = s.shape[-1]
    mover = int(s[2, 0, 0])
    if kind == 'suicide':
        return bool(invalid_moves(s)[q]) and group(s, seed)[1] == {q}
    t = s.copy()
    t[3] = 1
    t[3][q] = 0
    nxt, status = c_oracle.batch_next_states(t[None], np.array([q[0] * N + q[1]], np.int32))
    if status[0] or not every_group_has_a_liberty(nxt[0]):
        return False
    if kind == 'capture':
        return not nxt[0][1 - mover][seed]
    return len(group(nxt[0], seed)[1]) == {'atari': 1, 'join1': 1, 'join2': 2}[kind]


@functools.lru_cache(maxsize=None)
def cases(N):
    """-> states uint8 [K, 6, N, N], q int32 [K] (the forced action, -1 on boards that are not forced), point int32 [K] (the
    point the board is about: q, the suicide point, -1), kind (list of K names), seed int32 [K, 2] (a stone of the group under
    test - on join boards the point q, whose stone makes that group -, or -1), variant int32 [K] (orientation + 8 x white to
    move; the index on shape boards).  Ordered round by round, one board of every kind a round, so that the first few boards
    already hold every kind."""
    from oracle import c_oracle
    import test_gpu_adversarial
    per_kind = {k: [] for k in KINDS}
    for kind in TURNED:
        built = _grid(N, 'capture' if kind == 'corridor' else kind)
        if built is None:
            continue
        g, q0, seed0 = built
        for v in range(16):
            k, white = v & 7, v >> 3
            s = _state(turn(g, k), white)
            q, seed = turn_point(q0, k, N), turn_point(seed0, k, N)
            what = 'capture' if kind == 'corridor' else kind
            if N < 5 and not _fits(s, what, q, seed):
                continue
            if kind == 'suicide':
                s[3] = invalid_moves(s)
            else:
                s[3] = 1
                s[3][q] = 0
            a = q[0] * N + q[1]
            if kind == 'corridor':
                nxt, status = c_oracle.batch_next_states(s[None], np.array([a], np.int32))
                assert status[0] == 0
                per_kind[kind].append((nxt[0], -1, -1, seed, v))
            else:
                per_kind[kind].append((s, a if kind in FORCED else -1, a, seed, v))
    shapes = test_gpu_adversarial.consistent_boards(N)
    for i, s in enumerate(shapes):
        s[3] = invalid_moves(s)
        per_kind['shape'].append((s, -1, -1, (-1, -1), i))
    rows = []
    for rnd in range(max(len(v) for v in per_kind.values())):
        for i, kind in enumerate(KINDS):
            have = per_kind[kind]
            if rnd < len(have):
                # a round holds different variants of its kinds (the shapes are in an order of their own)
                rows.append((kind,) + have[(rnd + 3 * i) % len(have) if kind != 'shape' else rnd])
    return SimpleNamespace(states=np.stack([r[1] for r in rows]), q=np.array([r[2] for r in rows], np.int32),
                           point=np.array([r[3] for r in rows], np.int32), kind=[r[0] for r in rows],
                           seed=np.array([r[4] for r in rows], np.int32), variant=np.array([r[5] for r in rows], np.int32))


def positions(N, B0=BATCH):
    """the random positions of tests/test_gpu_dispatch_sizes.py (its child's positions(N)): three in four from the middle of a
    game, every fourth from games played on until most have ended"""
    from oracle import c_oracle
    z = np.zeros((B0, 6, N, N), np.uint8)
    mid, _, _ = c_oracle.batch_rollout_mt(z, c_oracle.rng_seed(100 + N, B0), N * N // 2 + 3, True, 16)
    late, _, _ = c_oracle.batch_rollout_mt(z[:B0 // 4], c_oracle.rng_seed(200 + N, B0 // 4), 3 * N * N, False, 16)
    mid[3::4] = late
    return mid


@functools.lru_cache(maxsize=None)
def batch(N):
    """The 256 boards every launch of the GPU test starts from (a launch of B boards takes the first B): three crafted boards,
    then one of positions(N), and so on - the crafted ones once through, then again (another generator each time) -, so one wave
    holds lanes that sweep many times next to lanes that are done at once.  -> states, q, kind ('random' on the others),
    index (into cases(N), -1 on the others)."""
    c, rand = cases(N), positions(N)
    K = len(c.kind)
    states, q, kind, index = rand.copy(), np.full(BATCH, -1, np.int32), ['random'] * BATCH, np.full(BATCH, -1, np.int32)
    j = 0
    for b in range(BATCH):
        if b % 4 != 3:
            states[b], q[b], kind[b], index[b] = c.states[j % K], c.q[j % K], c.kind[j % K], j % K
            j += 1
    return SimpleNamespace(states=states, q=q, kind=kind, index=index)


def rollout_batches(N):
    """the batch sizes of every rollout the GPU test launches at N: byte planes, tracked, packed, the eye-aware draw"""
    from test_gpu_dispatch_sizes import rollout_cells
    return sorted({B for B, _ in rollout_cells(N)} | {B for B, _ in TRACKED_CELLS + PACKED_CELLS + POLICY_CELLS})


TRACKED_CELLS = [(24, 1), (24, 3), (24, 9), (16, 1), (16, 3), (200, 1), (200, 3), (200, 9)]      # those of the dispatch test
PACKED_CELLS = [(200, 5), (30, 5), (30, 2)]
POLICY_CELLS = [(24, 9), (200, 9)]


def first_ply(N, B):
    """what the oracle draws on the first ply of a launch of B boards -> actions int32 [B]"""
    from oracle import c_oracle
    _, _, last = c_oracle.batch_rollout(batch(N).states[:B], c_oracle.rng_seed(SEED, B), 1, True)
    return last


def vertical_steps(stones, seed):
    """point -> the fewest vertical steps on a path inside `stones` from `seed` to it (0 - 1 search: a horizontal step is free)"""
    from collections import deque
    dist, todo = {seed: 0}, deque([seed])
    while todo:
        p = todo.popleft()
        for n, cost in (((p[0], p[1] - 1), 0), ((p[0], p[1] + 1), 0), ((p[0] - 1, p[1]), 1), ((p[0] + 1, p[1]), 1)):
            if n in stones and dist.get(n, 1 << 30) > dist[p] + cost:
                dist[n] = dist[p] + cost
                (todo.appendleft if cost == 0 else todo.append)(n)
    assert len(dist) == len(stones)
    return dist


def vertical_depth(stones, seed):
    """the fewest vertical steps on a path inside `stones` from `seed` to its farthest stone"""
    return max(vertical_steps(stones, seed).values())
