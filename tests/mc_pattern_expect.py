"""Expected results of the Monte Carlo stack under the `pattern` playout policy (gogame.batch_rollout_tracked, batch_playouts,
batch_move_playouts, batch_uct with policy='pattern'; gogame.batch_patterns), CPU only, built on tests/mc_tactics_expect.py and
the C restatement under oracle/: the thirteen patterns matched by brute force from their strings, the sets P and L in NumPy,
the playouts ply by ply with the previous move carried (the draw here, the move by the restatement's next_state over the live
boards), the reductions and the search as mc_expect has them.

The rule (include/gymgo_amd_pattern.h holds it word for word): P = the empty points whose eight neighbours match one of the
thirteen patterns in some view under either colouring; prev = the previous action if it is a point of the board; L = F and P and
the up to eight neighbours of prev.  With the gate of `tactical` open the ply draws from the first non-empty of C, E, L, F, with
it closed from F; the pass when the set is empty.  A reset ply, the ply after a pass and a job's first playout ply have no prev."""
import functools
import itertools

import numpy as np

import mc_expect as mc
import mc_policy_expect as mp
import mc_tactics_expect as mt
from oracle import c_oracle

PATTERNS = ('XOX/.../???', 'XO./.../?.?', 'XO?/X../x.?', '.O./X../...', 'XO?/O.o/?o?', 'XO?/O.X/???', '?X?/O.O/ooo',
            'OX?/o.O/???', 'X.?/O.?/###', 'OX?/X.O/###', '?X?/x.O/###', '?XO/x.x/###', '?OX/X.O/###')
COUNTS = (504, 256, 768, 8, 4544, 3392, 2812, 10304, 240, 64, 608, 504, 64)
TOTAL = 15828
EMPTY, BLACK, WHITE, OFF = 0, 1, 2, 3
SET_C, SET_E, SET_F, SET_L = mt.SET_C, mt.SET_E, mt.SET_F, 3
# the eight neighbours as (dy, dx), row by row: NW N NE W E SW S SE
NEIGH = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def _char_ok(ch, s, x, o):
    return {'X': s == x, 'O': s == o, '.': s == EMPTY, '#': s == OFF, '?': True, 'x': s != x, 'o': s != o}[ch]


def _views(rows):
    g = [list(r) for r in rows]
    out = []
    for _ in range(4):
        g = [[g[2 - c][r] for c in range(3)] for r in range(3)]
        out.append([''.join(r) for r in g])
        out.append([''.join(reversed(r)) for r in g])
    return out


def pattern_tables():
    """-> bool [13, 4^8]: entry [k, code] = the neighbourhood `code` (neighbour j of NEIGH in base-4 digit j: EMPTY, BLACK, WHITE,
    OFF) matches pattern k in some view under either colouring.  Brute force from the strings."""
    codes = np.array(list(itertools.product(range(4), repeat=8)), np.int8)[:, ::-1]   # digit j = neighbour j
    assert all(int((codes[c].astype(np.int64) * 4 ** np.arange(8)).sum()) == c for c in (0, 1, 4, 65535, 12345))
    out = np.zeros((len(PATTERNS), 4 ** 8), bool)
    for k, p in enumerate(PATTERNS):
        rows = p.split('/')
        assert rows[1][1] == '.'
        for v in _views(rows):
            for x, o in ((BLACK, WHITE), (WHITE, BLACK)):
                m = np.ones(4 ** 8, bool)
                for j, (dy, dx) in enumerate(NEIGH):
                    ok = np.array([_char_ok(v[1 + dy][1 + dx], s, x, o) for s in range(4)])
                    m &= ok[codes[:, j]]
                out[k] |= m
    return out


_TABLE = []


def match_table():
    """bool [4^8]: some pattern matches."""
    if not _TABLE:
        _TABLE.append(pattern_tables().any(axis=0))
    return _TABLE[0]


def neighbour_codes(states):
    """int64 [B, N, N]: the base-4 code of the eight neighbours of every point (pattern_tables' digits)."""
    states = np.asarray(states)
    col = np.where(states[:, 0] != 0, BLACK, np.where(states[:, 1] != 0, WHITE, EMPTY)).astype(np.int64)
    p = np.pad(col, ((0, 0), (1, 1), (1, 1)), constant_values=OFF)
    N = col.shape[1]
    code = np.zeros(col.shape, np.int64)
    for j, (dy, dx) in enumerate(NEIGH):
        code += p[:, 1 + dy:1 + dy + N, 1 + dx:1 + dx + N] * 4 ** j
    return code


def pattern_points(states):
    """P, bool [B, N, N]: the empty points that match; all False for a game that has ended."""
    states = np.asarray(states)
    empty = (states[:, 0] == 0) & (states[:, 1] == 0)
    ended = states[:, 5, 0, 0] != 0
    return empty & match_table()[neighbour_codes(states)] & ~ended[:, None, None]


def near_prev(last, B, N):
    """bool [B, N, N]: the up to eight on-board neighbours of the previous point; nothing where last is no point of the board."""
    out = np.zeros((B, N, N), bool)
    if last is None:
        return out
    last = np.asarray(last, np.int64).reshape(B)
    for b in np.flatnonzero((last >= 0) & (last < N * N)):
        y, x = divmod(int(last[b]), N)
        out[b, max(0, y - 1):y + 2, max(0, x - 1):x + 2] = True
        out[b, y, x] = False
    return out


def pattern_sets(states, last):
    """-> (P, L), bool [B, N, N] each (gogame.batch_patterns' two planes)."""
    states = np.asarray(states)
    B, _, N, _ = states.shape
    P = pattern_points(states)
    F = mt.tiers(states)[2]
    return P, F & P & near_prev(last, B, N)


def pattern_rollout(states, rng, plies, auto_reset=False, last=None, trace=None):
    """`plies` plies of the pattern policy on every game (gg_batch_rollout_tracked_policy3): -> (states, rng, last_actions int32
    [B] (-1: no ply played in this call), steps int64 [B]).  last (int32 [B] or None): the previous action of every board
    before the call.  trace (a list): gets one (live indices, boards before the ply, n, actions, set drawn from (SET_C / SET_E /
    SET_L / SET_F), gate open, (C empty and E empty and L not empty), previous action used, L) per ply."""
    cur = np.array(states, np.uint8, copy=True)
    rng = np.array(rng, np.uint64, copy=True)
    B, _, N, _ = cur.shape
    prev = np.full(B, -1, np.int64) if last is None else np.array(last, np.int64).reshape(B)
    out_last = np.full(B, -1, np.int32)
    steps = np.zeros(B, np.int64)
    for _ in range(int(plies)):
        done = cur[:, 5, 0, 0] != 0
        if auto_reset:
            cur[done] = 0
            prev[done] = -1
            live = np.arange(B)
        else:
            live = np.flatnonzero(~done)
        if live.size == 0:
            break
        sub = cur[live]
        n_live = len(live)
        C, E, F = (s.reshape(n_live, -1) for s in mt.tiers(sub))
        Lp = (F.reshape(n_live, N, N) & pattern_points(sub) & near_prev(prev[live], n_live, N)).reshape(n_live, -1)
        rng[live], u = mp.draw(rng[live])
        gate = (u & 3) != 0
        hasC, hasE, hasL = C.any(axis=1), E.any(axis=1), Lp.any(axis=1)
        which = np.where(gate & hasC, SET_C, np.where(gate & hasE, SET_E, np.where(gate & hasL, SET_L, SET_F)))
        cand = np.where((which == SET_C)[:, None], C, np.where((which == SET_E)[:, None], E, np.where((which == SET_L)[:, None], Lp, F)))
        n = cand.sum(axis=1).astype(np.int64)
        k = (u * n) >> 32
        order = np.cumsum(cand, axis=1) - 1
        hit = cand & (order == k[:, None])
        act = np.where(n > 0, hit.argmax(axis=1), N * N).astype(np.int32)
        if trace is not None:
            trace.append((live, sub.copy(), n, act.copy(), which, gate, ~hasC & ~hasE & hasL, prev[live].copy(), Lp.reshape(n_live, N, N)))
        nxt, status = c_oracle.batch_next_states(sub, act)
        assert not status.any()
        cur[live] = nxt
        out_last[live] = act
        prev[live] = act
        steps[live] += 1
    return cur, rng, out_last, steps


def trace_counts(trace):
    """-> dict: plies drawn from C / E / L / F over a trace, the plies whose gate was open with C and E empty and L not, the
    plies whose previous action was a pass, and the plies."""
    out = {'C': 0, 'E': 0, 'L': 0, 'F': 0, 'open_L_only': 0, 'after_pass': 0, 'plies': 0}
    for live, sub, _, _, which, gate, onlyL, prev, _ in trace:
        for name, code in (('C', SET_C), ('E', SET_E), ('L', SET_L), ('F', SET_F)):
            out[name] += int((which == code).sum())
        out['open_L_only'] += int((gate & onlyL).sum())
        out['after_pass'] += int((prev == sub.shape[2] ** 2).sum())
        out['plies'] += len(which)
    return out


# the restatements of mc_expect with the playouts played by pattern_rollout (policy='pattern'), every job from no previous
# point: a first move is not the playout's
expected_playouts_pattern = functools.partial(mc.expected_playouts, rollout=pattern_rollout)
expected_move_playouts_pattern = functools.partial(mc.expected_move_playouts, rollout=pattern_rollout)
expected_uct_pattern = functools.partial(mc.expected_uct, rollout=pattern_rollout)
playout_evaluator_np = functools.partial(mc.playout_evaluator_np, rollout=pattern_rollout)


# ---------------------------------------------------------------- hand-made positions
def crafted_positions():
    """-> list of (name, board uint8 [6, N, N], previous move (row, col), P, L as bool [N, N]) with the points of each set
    listed BY HAND (the issue's table): black to move and, colours swapped, white to move - the sets do not depend on it."""
    out = []

    def add(name, rows, prev, P, L):
        N = len(rows)
        for white in (False, True):
            b = mp.board(mp.swap_colours(rows) if white else rows, white)
            out.append((name + ('_white' if white else ''), b, prev, mt._pts(P, N), mt._pts(L, N)))

    p1 = [(0, 0), (0, 1), (0, 2), (2, 0), (2, 1), (2, 2)]
    add('hane_row', ['.....', 'BWB..', '.....', '.....', '.....'], (1, 1), p1, p1)
    p2 = [(0, 1), (0, 2), (2, 1), (2, 2)]
    add('pair', ['.....', '.BW..', '.....', '.....', '.....'], (1, 2), p2, p2)
    add('cut', ['.....', '.BW..', '.W...', '.....', '.....'], (2, 1), [(0, 1), (0, 2), (1, 0), (2, 0), (2, 2)], [(1, 0), (2, 0), (2, 2)])
    p4 = [(3, 0), (3, 2), (4, 0), (4, 2)]
    add('edge', ['.....', '.....', '.....', '.B...', '.W...'], (4, 1), p4, p4)
    add('two_by_two', ['BW', '..'], None, [(1, 0), (1, 1)], [])
    return out


def seam_roots():
    """19x19 roots whose previous move lies in rows 9 and 10 (the rows that split a k_rollout5 pair), rows 0 and 18, columns 0
    and 18 and the four corners, with an opponent stone beside it so that the shapes around it match: -> (roots uint8 [G, 6, 19,
    19], last int32 [G]).  The mover is the colour that did not play the previous move."""
    N = 19
    spots = [(9, 4), (10, 4), (9, 14), (10, 14), (0, 6), (18, 6), (7, 0), (7, 18), (0, 0), (0, 18), (18, 0), (18, 18)]
    roots, last = [], []
    for i, (y, x) in enumerate(spots):
        rows = [['.'] * N for _ in range(N)]
        rows[y][x] = 'W'                      # the previous move: white's, black to move
        dx = 1 if x + 1 < N else -1
        rows[y][x + dx] = 'B'                 # a black stone beside it: a hane / edge shape on either side
        dy = 1 if y + 1 < N else -1
        rows[y + dy][x + dx] = 'B' if i % 2 else '.'   # ... and on every second root one on the diagonal (no stone is in atari but the corners')
        text = [''.join(r) for r in rows]
        for white in (False, True):
            roots.append(mp.board(mp.swap_colours(text) if white else text, white))
            last.append(y * N + x)
    return np.stack(roots), np.array(last, np.int32)


# ---------------------------------------------------------------- the batches of tests/test_gpu_pattern.py
def last_cycle(N, B):
    """int32 [B]: previous actions that cycle over -1, the pass N^2, -7, 1 << 30, the corners, points of the edges and inner
    points."""
    P = N * N
    vals = [-1, P, -7, 1 << 30, 0, N - 1, P - N, P - 1, N // 2, (N // 2) * N, (N // 2) * N + N - 1, P - 1 - N // 2,
            (N // 2) * N + N // 2, N + 1, P - N - 2, (N - 2) * N + 1, 2 * N - 2]
    vals += list(range(0, P, max(1, P // 23)))
    return np.array([vals[i % len(vals)] for i in range(B)], np.int32)


def rollout_batch(N, B):
    """-> (states uint8 [B, 6, N, N], last int32 [B]): boards of mt.pool(N) over and over with last_cycle's previous actions - a
    previous action need not be a stone: the rule does not ask -, and at 19x19 the LAST boards are seam_roots() with their
    previous moves, in turn, as many as fit into half of the batch (at most 48): every copy has its own generator."""
    p = mt.pool(N)
    states = p[np.arange(B) % len(p)].copy()
    last = last_cycle(N, B)
    if N == 19:
        sr, sl = seam_roots()
        k = min(48, B // 2)
        states[B - k:] = sr[np.arange(k) % len(sr)]
        last[B - k:] = sl[np.arange(k) % len(sr)]
    return states, last
