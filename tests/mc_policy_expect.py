"""Expected results of the Monte Carlo stack under the `no_eye_fill` playout policy (gogame.batch_rollout_tracked, batch_playouts,
batch_move_playouts, batch_uct with policy='no_eye_fill'; gogame.batch_eye_mask), CPU only, built on tests/mc_expect.py and the
C restatement under oracle/: the rule itself in NumPy (eyes), the playouts ply by ply (the draw here, the move by the
restatement's next_state over the live boards), the reductions and the search as mc_expect has them."""
import functools

import numpy as np

import mc_expect as mc
from oracle import c_oracle

_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def eyes(states):
    """bool [B, N, N]: the eyes of the mover (plane 2) of every board [B, 6, N, N] - an empty point whose orthogonal neighbours
    on the board all hold a stone of the mover and of whose diagonal neighbours on the board at most one holds an opponent
    stone, none when the point lies on the first / last row or column.  All False for a game that has ended."""
    states = np.asarray(states)
    B, _, N, _ = states.shape
    white = states[:, 2, 0, 0] != 0
    me = np.where(white[:, None, None], states[:, 1], states[:, 0]) != 0
    op = np.where(white[:, None, None], states[:, 0], states[:, 1]) != 0
    edge = np.zeros((N, N), bool)
    edge[0] = edge[-1] = edge[:, 0] = edge[:, -1] = True
    mp = np.pad(me, ((0, 0), (1, 1), (1, 1)), constant_values=True)          # off-board counts as the mover's
    orth = mp[:, :-2, 1:-1] & mp[:, 2:, 1:-1] & mp[:, 1:-1, :-2] & mp[:, 1:-1, 2:]
    o = np.pad(op, ((0, 0), (1, 1), (1, 1)), constant_values=False).astype(np.int32)
    D = o[:, :-2, :-2] + o[:, :-2, 2:] + o[:, 2:, :-2] + o[:, 2:, 2:]
    eye = ~(me | op) & orth & np.where(edge[None], D == 0, D <= 1)
    ended = states[:, 5, 0, 0] != 0
    return eye & ~ended[:, None, None]


def candidates(states):
    """bool [B, N*N]: the points whose invalid bit (plane 3) is clear and that are not eyes of the mover."""
    states = np.asarray(states)
    B = states.shape[0]
    return ((states[:, 3] == 0) & ~eyes(states)).reshape(B, -1)


def draw(rng):
    """One step of the per-game generators (uint64 [B]) -> (the generators after it, the high 32 bits of the draw as int64)."""
    with np.errstate(over='ignore'):
        x = rng + np.uint64(mc.GOLDEN_GAMMA)
        z = (x ^ (x >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        z = z ^ (z >> np.uint64(31))
    return x, (z >> np.uint64(32)).astype(np.int64)


def policy_rollout(states, rng, plies, auto_reset=False, trace=None):
    """`plies` plies of the no_eye_fill policy on every game (gg_batch_rollout_tracked_policy): -> (states, rng, last_actions
    int32 [B] (-1: no ply played), steps int64 [B]).  A finished game is reset first when auto_reset, else it stays as it is
    and its generator does not move.  trace (a list): gets one (live indices, boards before the ply, n, actions) per ply."""
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
        cand = candidates(sub)
        n = cand.sum(axis=1).astype(np.int64)
        rng[live], u = draw(rng[live])
        k = (u * n) >> 32                                         # floor((u >> 32) n / 2^32); u < 2^32, n <= 361
        order = np.cumsum(cand, axis=1) - 1                       # rank of every candidate
        hit = cand & (order == k[:, None])
        act = np.where(n > 0, hit.argmax(axis=1), N * N).astype(np.int32)
        if trace is not None:
            trace.append((live, sub.copy(), n, act.copy()))
        nxt, status = c_oracle.batch_next_states(sub, act)
        assert not status.any()
        cur[live] = nxt
        last[live] = act
        steps[live] += 1
    return cur, rng, last, steps


# the restatements of mc_expect with the playouts played by policy_rollout (batch_playouts / batch_move_playouts / batch_uct with
# policy='no_eye_fill': every legal first move and every legal action of the tree stay, eyes included)
expected_playouts_policy = functools.partial(mc.expected_playouts, rollout=policy_rollout)
expected_move_playouts_policy = functools.partial(mc.expected_move_playouts, rollout=policy_rollout)
expected_uct_policy = functools.partial(mc.expected_uct, rollout=policy_rollout)


# ---------------------------------------------------------------- crafted positions
def board(rows, white_to_move=False):
    """A position from strings ('B', 'W', '.'), black to move unless told otherwise, with its invalid-move plane."""
    N = len(rows)
    st = np.zeros((6, N, N), np.uint8)
    for y, row in enumerate(rows):
        assert len(row) == N
        for x, ch in enumerate(row):
            if ch != '.':
                st[0 if ch == 'B' else 1, y, x] = 1
    st[2] = 1 if white_to_move else 0
    st[3] = c_oracle.compute_invalid_moves(st, 0 if white_to_move else 1)   # (the restatement's `player`: who moved LAST)
    return st


def swap_colours(rows):
    return [r.replace('B', 'x').replace('W', 'B').replace('x', 'W') for r in rows]


# (name, rows, the eyes of BLACK to move as (row, col))
CRAFTED = [
    ('centre', ['.....', '..B..', '.B.B.', '..B..', '.....'], [(2, 2)]),
    ('centre_one_diagonal', ['.....', '.WB..', '.B.B.', '..B..', '.....'], [(2, 2)]),
    ('centre_two_diagonals', ['.....', '.WB..', '.B.B.', '..BW.', '.....'], []),
    ('edge', ['.B.B.', '..B..', '.....', '.....', '.....'], [(0, 2)]),
    ('edge_one_diagonal', ['.B.B.', '.WB..', '.....', '.....', '.....'], []),
    ('corner', ['.B...', 'B....', '.....', '.....', '.....'], [(0, 0)]),
    ('corner_one_diagonal', ['.B...', 'BW...', '.....', '.....', '.....'], []),
    ('open_neighbour', ['.....', '..B..', '.B.B.', '.....', '.....'], []),
    ('two_by_two', ['.B', 'B.'], [(0, 0), (1, 1)]),
    ('last_row_and_column', ['.....', '.....', '....B', '...B.', '..B.B'], [(4, 3), (3, 4)]),
]


def crafted_eye_boards():
    """-> (boards list of uint8 [6, N, N], expected eye masks list of bool [N, N]): CRAFTED with black to move, then the same
    with the colours swapped and white to move."""
    boards, want = [], []
    for white in (False, True):
        for _, rows, pts in CRAFTED:
            boards.append(board(swap_colours(rows) if white else rows, white))
            m = np.zeros((len(rows), len(rows)), bool)
            for y, x in pts:
                m[y, x] = True
            want.append(m)
    return boards, want


def seam_roots():
    """19x19 roots, black to move, with a black eye in the first and the last row that each lane of a k_rollout5 pair holds
    (rows 0, 9, 10, 18) and white stones elsewhere so that the game goes on."""
    N = 19
    rows = [['.'] * N for _ in range(N)]
    def eye(y, x):
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            if 0 <= y + dy < N and 0 <= x + dx < N:
                rows[y + dy][x + dx] = 'B'
    eye(0, 3)
    eye(9, 6)
    eye(10, 12)
    eye(18, 15)
    for x in range(0, N, 2):
        rows[14][x] = 'W'
    a = board([''.join(r) for r in rows])
    e = eyes(a[None])[0]
    assert e[0, 3] and e[9, 6] and e[10, 12] and e[18, 15]
    b = board(swap_colours([''.join(r) for r in rows]), True)
    return np.stack([a, b])


def forced_pass_roots(N):
    """Roots where the mover has no candidate: black owns the whole board but two one-point eyes (both are eyes: the pass is
    forced), black to move; and the same position with white to move, whose only legal points are suicides - none."""
    rows = [['B'] * N for _ in range(N)]
    rows[0][0] = '.'
    rows[N - 1][N - 1] = '.'
    rows = [''.join(r) for r in rows]
    a = board(rows)
    assert candidates(a[None]).sum() == 0 and (a[3] == 0).sum() == 2
    b = board(rows, True)
    assert candidates(b[None]).sum() == 0
    return np.stack([a, b])
