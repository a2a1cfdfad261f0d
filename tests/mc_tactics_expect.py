"""Expected results of the Monte Carlo stack under the `tactical` playout policy (gogame.batch_rollout_tracked, batch_playouts,
batch_move_playouts, batch_uct with policy='tactical'; gogame.batch_tactics), CPU only, built on tests/mc_policy_expect.py and
the C restatement under oracle/: the rule itself in NumPy (tiers), the playouts ply by ply (the draw here, the move by the
restatement's next_state over the live boards), the reductions and the search as mc_expect has them.

The rule (include/gymgo_amd_tactics.h holds it word for word): low = the stones whose group has fewer than two liberties,
valid = the points whose invalid bit is clear; C = valid points next to an opponent stone in low, E = valid points next to a
mover's stone in low with at least two empty neighbours, F = valid points that are not eyes of the mover.  With u the high 32
bits of the ply's draw the gate is open when (u & 3) != 0; the set is C if the gate is open and C is not empty, else E if the
gate is open and E is not empty, else F; the pass when it is empty, else its floor(u n / 2^32)-th point."""
import functools

import numpy as np

import mc_expect as mc
import mc_policy_expect as mp
from oracle import c_oracle

SET_C, SET_E, SET_F = 0, 1, 2


def _shifted(a, fill):
    """The four orthogonal neighbours of every point of a [B, N, N]: up, down, left, right; `fill` off the board."""
    p = np.pad(a, ((0, 0), (1, 1), (1, 1)), constant_values=fill)
    return p[:, :-2, 1:-1], p[:, 2:, 1:-1], p[:, 1:-1, :-2], p[:, 1:-1, 2:]


def group_liberty_counts(states):
    """int32 [B, N, N]: the number of liberties of the group of the stone at every point, 0 at empty points - per group, by
    label propagation over the whole batch at once (features_expect.group_liberties gives the same board by board:
    tests/test_tactics_host.py holds the two together, and takes `low` of the hand-made positions from that one)."""
    states = np.asarray(states)
    B, _, N, _ = states.shape
    P = N * N
    bl, wh = states[:, 0] != 0, states[:, 1] != 0
    stones = bl | wh
    col = np.where(bl, 1, np.where(wh, 2, 0)).astype(np.int8)
    big = np.int32(P)
    lab = np.where(stones, np.arange(P, dtype=np.int32).reshape(1, N, N), big)
    while True:
        new = lab
        for nl, nc in zip(_shifted(lab, big), _shifted(col, 0)):
            new = np.minimum(new, np.where((nc == col) & stones, nl, big))
        if np.array_equal(new, lab):
            break
        lab = new
    empty = ~stones
    idx = np.arange(P, dtype=np.int64).reshape(1, N, N)
    keys = []
    for nl in _shifted(lab, big):                       # an empty point and the group of the stone next to it
        m = empty & (nl < big)
        b = np.nonzero(m)[0].astype(np.int64)
        keys.append((b * (P + 1) + nl[m]) * P + np.broadcast_to(idx, m.shape)[m])
    keys = np.unique(np.concatenate(keys))
    grp, cnt = np.unique(keys // P, return_counts=True)
    table = np.zeros(B * (P + 1), np.int32)
    table[grp] = cnt
    return np.where(stones, table[np.arange(B, dtype=np.int64)[:, None, None] * (P + 1) + lab], 0).astype(np.int32)


def low_stones(states, counts=None):
    """bool [B, N, N]: the stones of either colour whose group has fewer than two liberties."""
    states = np.asarray(states)
    c = group_liberty_counts(states) if counts is None else counts
    return ((states[:, 0] != 0) | (states[:, 1] != 0)) & (c < 2)


def tiers(states, counts=None):
    """-> (C, E, F), bool [B, N, N] each: the capture points, the escape points and the candidates of no_eye_fill of the mover
    of every board [B, 6, N, N].  All False for a game that has ended.  counts: the per-group liberty counts to take `low`
    from (default: group_liberty_counts)."""
    states = np.asarray(states)
    white = states[:, 2, 0, 0] != 0
    me = np.where(white[:, None, None], states[:, 1], states[:, 0]) != 0
    op = np.where(white[:, None, None], states[:, 0], states[:, 1]) != 0
    low = low_stones(states, counts)
    ended = states[:, 5, 0, 0] != 0
    valid = (states[:, 3] == 0) & ~ended[:, None, None]
    near = lambda s: np.logical_or.reduce(_shifted(s, False))
    empties = sum(x.astype(np.int32) for x in _shifted(~(me | op), False))       # the border is never empty
    C = valid & near(op & low)
    E = valid & near(me & low) & (empties >= 2)
    F = valid & ~mp.eyes(states)
    return C, E, F


def tactical_rollout(states, rng, plies, auto_reset=False, trace=None):
    """`plies` plies of the tactical policy on every game (gg_batch_rollout_tracked_policy2): -> (states, rng, last_actions
    int32 [B] (-1: no ply played), steps int64 [B]); the shape of mc_policy_expect.policy_rollout.  trace (a list): gets one
    (live indices, boards before the ply, n, actions, set drawn from (SET_C / SET_E / SET_F), gate open, C not empty) per ply."""
    cur = np.array(states, np.uint8, copy=True)
    rng = np.array(rng, np.uint64, copy=True)
    B, _, N, _ = cur.shape
    last = np.full(B, -1, np.int32)
    steps = np.zeros(B, np.int64)
    for _ in range(int(plies)):
        done = cur[:, 5, 0, 0] != 0
        if auto_reset:
            cur[done] = 0
            live = np.arange(B)
        else:
            live = np.flatnonzero(~done)
        if live.size == 0:
            break
        sub = cur[live]
        C, E, F = (s.reshape(len(live), -1) for s in tiers(sub))
        rng[live], u = mp.draw(rng[live])
        gate = (u & 3) != 0
        hasC, hasE = C.any(axis=1), E.any(axis=1)
        which = np.where(gate & hasC, SET_C, np.where(gate & hasE, SET_E, SET_F))
        cand = np.where((which == SET_C)[:, None], C, np.where((which == SET_E)[:, None], E, F))
        n = cand.sum(axis=1).astype(np.int64)
        k = (u * n) >> 32
        order = np.cumsum(cand, axis=1) - 1
        hit = cand & (order == k[:, None])
        act = np.where(n > 0, hit.argmax(axis=1), N * N).astype(np.int32)
        if trace is not None:
            trace.append((live, sub.copy(), n, act.copy(), which, gate, hasC))
        nxt, status = c_oracle.batch_next_states(sub, act)
        assert not status.any()
        cur[live] = nxt
        last[live] = act
        steps[live] += 1
    return cur, rng, last, steps


def trace_counts(trace):
    """-> dict: plies drawn from C / E / F over a trace, and the plies with a closed gate while C was not empty."""
    out = {'C': 0, 'E': 0, 'F': 0, 'closed_with_C': 0, 'plies': 0}
    for _, _, _, _, which, gate, hasC in trace:
        out['C'] += int((which == SET_C).sum())
        out['E'] += int((which == SET_E).sum())
        out['F'] += int((which == SET_F).sum())
        out['closed_with_C'] += int((~gate & hasC).sum())
        out['plies'] += len(which)
    return out


# the restatements of mc_expect with the playouts played by tactical_rollout (policy='tactical')
expected_playouts_tactical = functools.partial(mc.expected_playouts, rollout=tactical_rollout)
expected_move_playouts_tactical = functools.partial(mc.expected_move_playouts, rollout=tactical_rollout)
expected_uct_tactical = functools.partial(mc.expected_uct, rollout=tactical_rollout)
playout_evaluator_np = functools.partial(mc.playout_evaluator_np, rollout=tactical_rollout)


# ---------------------------------------------------------------- hand-made positions
def _pts(points, N):
    m = np.zeros((N, N), bool)
    for y, x in points:
        m[y, x] = True
    return m


def crafted_positions():
    """-> list of (name, board uint8 [6, N, N], C, E as bool [N, N]) with the points of each set listed BY HAND, black to move
    and, colours swapped, white to move; F is the candidates of no_eye_fill (mc_policy_expect).  Every board's invalid plane
    comes from the restatement, the ko board from a played-out ko."""
    out = []

    def add(name, rows, C, E):
        N = len(rows)
        for white in (False, True):
            b = mp.board(mp.swap_colours(rows) if white else rows, white)
            out.append((name + ('_white' if white else ''), b, _pts(C, N), _pts(E, N)))

    # captures in the centre, on an edge, in a corner (white's lone stone has one liberty)
    add('capture_centre', ['.....', '..B..', '.BW..', '..B..', '.....'], [(2, 3)], [])
    add('capture_edge', ['.BW..', '..B..', '.....', '.....', '.....'], [(0, 3)], [])
    add('capture_corner', ['WB...', '.....', '.....', '.....', '.....'], [(1, 0)], [])
    # two white groups, (2, 1) and (2, 3), each with the one liberty (2, 2): one move takes both
    add('capture_two_groups', ['.....', '.B.B.', 'BW.WB', '.B.B.', '.....'], [(2, 2)], [])
    # black (1, 2) in atari, last liberty (2, 2): its neighbours are (1, 2) black, (3, 2) white, (2, 1) white, (2, 3) EMPTY -
    # exactly one empty neighbour: not an escape
    add('escape_one_empty', ['..W..', '.WBW.', '.W...', '..W..', '.....'], [], [])
    # black (2, 2) in atari, last liberty (2, 3) with the empty neighbours (1, 3), (3, 3), (2, 4): an escape; with exactly
    # two: white on (1, 3)
    add('escape_three_empty', ['.....', '..W..', '.WB..', '..W..', '.....'], [], [(2, 3)])
    add('escape_two_empty', ['.....', '..WW.', '.WB..', '..W..', '.....'], [], [(2, 3)])
    # black (2, 1) and white (2, 2) both in atari: white's neighbours are (1, 2) B, (3, 2) B, (2, 1) B and its last liberty
    # (2, 3) - a capture; black's are (1, 1) W, (3, 1) W, (2, 2) W and its last liberty (2, 0) with the empty neighbours
    # (1, 0) and (3, 0) - an escape
    add('capture_and_escape_apart', ['.....', '.WB..', '.BW..', '.WB..', '.....'], [(2, 3)], [(2, 0)])
    # an escape that is also a capture: black (1, 1) in atari with the last liberty (1, 2), which is also the last liberty of
    # white (1, 3); (1, 2) has the empty neighbours (0, 2) and (2, 2): in C (and in E: the set drawn from is C)
    add('escape_is_capture', ['.W.B.', 'WB.WB', '.W.B.', '.....', '.....'], [(1, 2)], [(1, 2)])
    # the ko: crafted_roots' ko root, white to move, may not retake at KO_POINT although the black stone (1, 2) is in atari
    ko = mc.crafted_roots(5)[2]
    assert ko[3, 1, 1] == 1 and ko[2].all()
    out.append(('ko_point_not_in_C', ko, _pts([], 5), _pts([], 5)))
    return out


def seam_roots():
    """19x19 roots with groups of both colours in atari whose last liberty lies across the rows 9 | 10 that split a k_rollout5
    pair (the stone in row 9 and its liberty in row 10, and the other way round), in rows 0 and 18 and in columns 0 and 18;
    black to move, and the colour-swapped form with white to move.  Every last liberty is a capture point or - with two empty
    neighbours - an escape point of the mover."""
    N = 19
    rows = [['.'] * N for _ in range(N)]

    def atari(y, x, c, lib):
        """a stone of colour c at (y, x) whose neighbours other than `lib` hold the other colour"""
        rows[y][x] = c
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            q = (y + dy, x + dx)
            if 0 <= q[0] < N and 0 <= q[1] < N and q != lib:
                rows[q[0]][q[1]] = 'B' if c == 'W' else 'W'

    libs = []
    for c, x0 in (('W', 2), ('B', 11)):
        atari(9, x0, c, (10, x0)); libs.append((10, x0))           # the stone in row 9, its liberty across the seam in row 10
        atari(10, x0 + 4, c, (9, x0 + 4)); libs.append((9, x0 + 4))   # ... and the other way round
    atari(1, 4, 'W', (0, 4)); libs.append((0, 4))                  # last liberty in row 0
    atari(1, 13, 'B', (0, 13)); libs.append((0, 13))
    atari(17, 4, 'W', (18, 4)); libs.append((18, 4))               # ... in row 18
    atari(17, 13, 'B', (18, 13)); libs.append((18, 13))
    atari(4, 1, 'W', (4, 0)); libs.append((4, 0))                  # ... in column 0
    atari(14, 1, 'B', (14, 0)); libs.append((14, 0))
    atari(4, 17, 'W', (4, 18)); libs.append((4, 18))               # ... in column 18
    atari(14, 17, 'B', (14, 18)); libs.append((14, 18))
    text = [''.join(r) for r in rows]
    a = mp.board(text)
    b = mp.board(mp.swap_colours(text), True)
    roots = np.stack([a, b])
    counts = group_liberty_counts(roots)
    C, E, _ = tiers(roots)
    for i in range(2):
        for y, x in libs:
            assert C[i, y, x] or E[i, y, x], (i, y, x)
        assert C[i, 10, 2] and C[i, 9, 6] and E[i, 10, 11] and E[i, 9, 15], i     # both directions, both colours
        assert C[i, 0, 4] and C[i, 18, 4] and C[i, 4, 0] and C[i, 4, 18], i
    assert (counts[0][np.array([9, 10, 9, 10]), np.array([2, 6, 11, 15])] == 1).all()
    return roots


# ---------------------------------------------------------------- the batches of tests/test_gpu_tactics.py
def pool(N):
    """Roots of every kind at size N: positions of random play (the last one a finished game), mc_cases' named roots (mid-game
    and late roots, the empty board, a root after a pass, a ko root for N >= 4, finished games, roots whose mover has no
    candidate) and, at 5x5, the hand-made positions of crafted_positions()."""
    import mc_cases as cs
    parts = [cs.stack(N), mc.make_roots(N, 24, 5 + N, max_ply=2 * N * N, step=max(2, N * N // 12))]
    if N == 5:
        parts.append(np.stack([p[1] for p in crafted_positions()]))
    return np.concatenate(parts)


def rollout_batch(N, B):
    """B boards of pool(N), over and over; at 19x19 the LAST boards are the two seam_roots() in turn, 22 times each (as many
    as fit into half of a small batch): every copy has its own generator, so the gate is open on the first ply of some copy
    of either root with near certainty (1 - 4^-22)."""
    p = pool(N)
    states = p[np.arange(B) % len(p)].copy()
    if N == 19:
        seam = seam_roots()
        k = min(44, B // 2)
        states[B - k:] = seam[np.arange(k) % 2]
    return states
