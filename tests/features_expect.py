"""Expected network input planes and per-group liberty counts (gogame.batch_features, batch_features_tracked,
batch_group_liberties), written the slow definitional way: CPU only, NumPy only, a breadth-first search per group, a SET of
liberty points per group, then the sixteen planes and the count plane point by point from the table of
include/gymgo_amd.h.  Shares no code with the kernels or with oracle/."""
from collections import deque

import numpy as np

PLANES = 16
NAMES = ('own', 'opponent', 'own_libs_1', 'own_libs_2', 'own_libs_3', 'own_libs_4plus', 'opp_libs_1', 'opp_libs_2',
         'opp_libs_3', 'opp_libs_4plus', 'legal', 'ko', 'capture', 'black_to_move', 'prev_pass', 'ones')


def neighbours(y, x, N):
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        if 0 <= y + dy < N and 0 <= x + dx < N:
            yield y + dy, x + dx


def groups(state):
    """-> (gid int [N, N]: the group of the stone at each point, -1 at empty points; libs: per group the set of its liberty
    points).  A group: a maximal orthogonally connected set of stones of one colour."""
    N = state.shape[-1]
    colour = np.where(state[0] != 0, 0, np.where(state[1] != 0, 1, -1))
    gid = np.full((N, N), -1, int)
    libs = []
    for y0 in range(N):
        for x0 in range(N):
            if colour[y0, x0] < 0 or gid[y0, x0] >= 0:
                continue
            g = len(libs)
            mine = set()
            gid[y0, x0] = g
            todo = deque([(y0, x0)])
            while todo:
                y, x = todo.popleft()
                for ny, nx in neighbours(y, x, N):
                    if colour[ny, nx] < 0:
                        mine.add((ny, nx))
                    elif colour[ny, nx] == colour[y0, x0] and gid[ny, nx] < 0:
                        gid[ny, nx] = g
                        todo.append((ny, nx))
            libs.append(mine)
    return gid, libs


def group_liberties(state):
    """uint8 [N, N]: the number of liberties of the group of the stone at each point, saturated at 255; 0 at empty points."""
    gid, libs = groups(state)
    N = state.shape[-1]
    out = np.zeros((N, N), np.uint8)
    for y in range(N):
        for x in range(N):
            if gid[y, x] >= 0:
                out[y, x] = min(len(libs[gid[y, x]]), 255)
    return out


def features(state):
    """uint8 [16, N, N] of one state [6, N, N]."""
    N = state.shape[-1]
    white_to_move = bool(state[2, 0, 0])
    passed, done = bool(state[4, 0, 0]), bool(state[5, 0, 0])
    own, opp = (state[1], state[0]) if white_to_move else (state[0], state[1])
    gid, libs = groups(state)
    out = np.zeros((PLANES, N, N), np.uint8)
    for y in range(N):
        for x in range(N):
            is_own, is_opp = own[y, x] != 0, opp[y, x] != 0
            out[0, y, x], out[1, y, x] = is_own, is_opp
            if is_own or is_opp:
                n = len(libs[gid[y, x]])
                k = 0 if n == 0 else min(n, 4)
                if k:
                    out[(2 if is_own else 6) + k - 1, y, x] = 1
                continue
            # an empty point
            atari = any(opp[ny, nx] != 0 and len(libs[gid[ny, nx]]) == 1 for ny, nx in neighbours(y, x, N))
            invalid = state[3, y, x] != 0
            legal = not invalid and not done
            out[10, y, x] = legal
            out[11, y, x] = invalid and not done and atari
            out[12, y, x] = legal and atari
    out[13] = 0 if white_to_move else 1
    out[14] = 1 if passed else 0
    out[15] = 1
    return out


def batch_features(states):
    states = np.asarray(states)
    return np.stack([features(s) for s in states]) if len(states) else np.zeros((0, PLANES) + states.shape[2:], np.uint8)


def batch_group_liberties(states):
    states = np.asarray(states)
    return np.stack([group_liberties(s) for s in states]) if len(states) else np.zeros((0,) + states.shape[2:], np.uint8)


# ---------------------------------------------------------------- boards for the tests
def board(rows, white_to_move=False, passed=False, done=False, invalid=()):
    """uint8 [6, N, N] from N strings of 'X' (black), 'O' (white), '.'; plane 3 = the stones + the points of `invalid`
    (hand-made boards carry the mask their author gives them: the planes take it as given)."""
    N = len(rows)
    s = np.zeros((6, N, N), np.uint8)
    for y, row in enumerate(rows):
        assert len(row) == N, rows
        for x, ch in enumerate(row):
            if ch == 'X':
                s[0, y, x] = 1
            elif ch == 'O':
                s[1, y, x] = 1
    s[3] = s[0] | s[1]
    for y, x in invalid:
        s[3, y, x] = 1
    s[2] = 1 if white_to_move else 0
    s[4] = 1 if passed else 0
    s[5] = 1 if done else 0
    return s


def spiral(N):
    """One black group that winds around the board from the rim inwards, with a one-point-wide empty channel between its
    turns: the longest flood an N x N board holds."""
    g = [['.'] * N for _ in range(N)]
    y, x, dy, dx = 0, 0, 0, 1
    g[0][0] = 'X'
    turns = 0
    while turns < 2:
        ny, nx = y + dy, x + dx
        ay, ax = ny + dy, nx + dx          # the point after the next: a stone there would close the channel
        ok = 0 <= ny < N and 0 <= nx < N and g[ny][nx] == '.' and not (0 <= ay < N and 0 <= ax < N and g[ay][ax] == 'X')
        if ok:
            # the next point must not touch the spiral sideways either (only the point it comes from)
            for sy, sx in neighbours(ny, nx, N):
                if (sy, sx) != (y, x) and g[sy][sx] == 'X':
                    ok = False
        if ok:
            y, x = ny, nx
            g[y][x] = 'X'
            turns = 0
        else:
            dy, dx = dx, -dy               # turn right
            turns += 1
    return [''.join(r) for r in g]


def comb(N):
    """One black group: the top row and every other column hanging from it down to the last row but one - its liberties
    are the channels between the teeth and the row below them (more than 128 on 19x19)."""
    rows = ['X' * N]
    for y in range(1, N - 1):
        rows.append(''.join('X' if x % 2 == 0 else '.' for x in range(N)))
    rows.append('.' * N)
    return rows


def crafted(N):
    """The hand-made boards of the GPU test at size N (9 or 19), each with black and with white to move -> uint8 [.., 6, N, N]."""
    out = []
    dot = '.' * N
    # stones in column 0 of row r and column N - 1 of row r - 1 are not neighbours
    wrap = [dot] * N
    wrap[3] = '.' * (N - 1) + 'X'
    wrap[4] = 'X' + '.' * (N - 1)
    wrap[6] = '.' * (N - 1) + 'O'
    wrap[7] = 'X' + '.' * (N - 1)
    # groups with exactly 3 and exactly 4 liberties side by side (and 2, and 5, around them)
    side = [dot] * N
    side[0] = 'X.O' + '.' * (N - 3)                 # corner stone: 2; edge stone: 3
    side[2] = '.XO.XX' + '.' * (N - 6)              # 3 | 3 ... and a pair with 6
    side[3] = '......X' + '.' * (N - 7)             # 3 ...
    side[4] = 'XO..XOO' + '.' * (N - 7)             # edge 2 | 3, then 3 next to a pair with exactly 4
    side[6] = '..X.O..' + '.' * (N - 7)             # 4 and 4
    side[7] = '...X...' + '.' * (N - 7)             # 4 (diagonal to both: no neighbour)
    # a board full but for two points
    fullb = ['X' * N for _ in range(N)]
    fullb[0] = '.' + 'X' * (N - 1)
    fullb[N - 1] = 'X' * (N - 1) + '.'
    fullw = ['XO' * (N // 2) + 'X' for _ in range(N)]
    fullw[N // 2] = '.' + fullw[N // 2][1:-1] + '.'
    for rows in (spiral(N), comb(N), wrap, side, fullb, fullw, [dot] * N):
        for white in (False, True):
            out.append(board(rows, white_to_move=white))
    return np.stack(out)
