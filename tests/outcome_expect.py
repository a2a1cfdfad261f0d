"""Expected move-outcome counts and planes (gogame.batch_move_counts, batch_move_planes, batch_move_planes_tracked), written
the slow definitional way: CPU only, NumPy only, the move played on a copy of the board and a breadth-first search per chain,
point by point from the definition of include/gymgo_amd.h.  Shares no code with the kernels or with oracle/.  Also the
hand-made boards of the tests (CRAFTED), each with the counts it was drawn for."""
import functools
from collections import deque
from types import SimpleNamespace

import numpy as np

import features_expect as fe

PLANES = 12
COUNTS = 3
NAMES = ('libs_after_1', 'libs_after_2', 'libs_after_3', 'libs_after_4plus', 'captures_1', 'captures_2', 'captures_3',
         'captures_4plus', 'self_atari_1', 'self_atari_2', 'self_atari_3', 'self_atari_4plus')
EMPTY, OWN, OPP = 0, 1, 2


def chain(grid, y0, x0):
    """-> (the stones of the chain of the stone at (y0, x0), its liberty points), two sets."""
    N = grid.shape[0]
    colour = grid[y0, x0]
    stones, libs, todo = {(y0, x0)}, set(), deque([(y0, x0)])
    while todo:
        y, x = todo.popleft()
        for q in fe.neighbours(y, x, N):
            if grid[q] == EMPTY:
                libs.add(q)
            elif grid[q] == colour and q not in stones:
                stones.add(q)
                todo.append(q)
    return stones, libs


def candidates(state):
    """bool [N, N]: empty, plane 3 clear, game not over."""
    s = np.asarray(state)
    if s[5, 0, 0]:
        return np.zeros(s.shape[1:], bool)
    return (s[0] == 0) & (s[1] == 0) & (s[3] == 0)


def candidates_of(states):
    """bool [B, N, N]: candidates() of every board."""
    return np.stack([candidates(s) for s in np.asarray(states)])


def play(state, y, x):
    """The mover's stone on the empty point (y, x) -> (libs, captured, size, joined): the liberties of the stone's chain after
    the opponent chains without a liberty have left, the stones that left, the chain's stones - all 0 for a suicide - and the
    number of own chains next to the point before the move."""
    s = np.asarray(state)
    N = s.shape[-1]
    white = bool(s[2, 0, 0])
    own, opp = (s[1], s[0]) if white else (s[0], s[1])
    grid = np.where(own != 0, OWN, np.where(opp != 0, OPP, EMPTY))
    assert grid[y, x] == EMPTY
    joined = []
    for q in fe.neighbours(y, x, N):
        if grid[q] == OWN and not any(q in c for c in joined):
            joined.append(chain(grid, *q)[0])
    grid[y, x] = OWN
    captured = set()
    for q in fe.neighbours(y, x, N):
        if grid[q] == OPP and q not in captured:
            stones, libs = chain(grid, *q)
            if not libs:
                captured |= stones
    for q in captured:
        grid[q] = EMPTY
    stones, libs = chain(grid, y, x)
    if not libs:
        return 0, 0, 0, len(joined)
    return len(libs), len(captured), len(stones), len(joined)


def outcome(state):
    """int [4, N, N]: libs, captured, size (not saturated) and the own chains joined, 0 at every point that is no candidate."""
    s = np.asarray(state)
    out = np.zeros((4,) + s.shape[1:], int)
    for y, x in np.argwhere(candidates(s)):
        out[:, y, x] = play(s, y, x)
    return out


def counts_of(raw):
    """uint8 [.., 3, N, N] from outcome(): saturated at 255."""
    return np.minimum(raw[..., :COUNTS, :, :], 255).astype(np.uint8)


def planes_of(raw):
    """uint8 [.., 12, N, N] from outcome(): the table of include/gymgo_amd.h."""
    libs, cap, size = (np.minimum(raw[..., k, :, :], 4) for k in range(COUNTS))
    rows = [libs == k for k in (1, 2, 3, 4)] + [cap == k for k in (1, 2, 3, 4)] + [(libs == 1) & (size == k) for k in (1, 2, 3, 4)]
    return np.stack(rows, axis=-3).astype(np.uint8)


def batch_outcome(states):
    states = np.asarray(states)
    return np.stack([outcome(s) for s in states]) if len(states) else np.zeros((0, 4) + states.shape[2:], int)


def batch_counts(states):
    return counts_of(batch_outcome(states))


def batch_planes(states):
    return planes_of(batch_outcome(states))


@functools.lru_cache(maxsize=None)
def case(N, kind):
    """The set `kind` of tests/plane_cases.py at size N with its expectation, computed once: .states, .raw [B, 4, N, N],
    .counts [B, 3, N, N], .planes [B, 12, N, N].  Read only."""
    import plane_cases as pc
    s = pc.states_of(N, kind)
    raw = batch_outcome(s)
    c = SimpleNamespace(N=N, kind=kind, states=s, raw=raw, counts=counts_of(raw), planes=planes_of(raw))
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---------------------------------------------------------------- hand-made boards
def _full19(rows_black, white_row=None):
    rows = ['X' * 19 if y < rows_black else '.' * 19 for y in range(19)]
    rows[0] = '.' + rows[0][1:]
    if white_row is not None:
        rows[white_row] = 'O' * 19
    return rows


_SNAPBACK = ['XOX.X',
             'XOOOX',
             '.XXX.',
             '.....',
             '.....']
_JOIN = ['OXOXO',
         'OX.XO',
         '.OOO.',
         '.....',
         '.....']
_EDGES = ['OXXOX..',
          '.......',
          '.......',
          '.......',
          '.......',
          '.......',
          '.......']
_KO = ['.XO..',
       'XO.O.',
       '.XO..',
       '.....',
       '.....']
_SUICIDE = ['.O...',
            'O....',
            '.....',
            '.....',
            '.....']
# (name, board, [(y, x, (libs, captured, size))]): the counts, not saturated, each board was drawn for
CRAFTED = (
    # white takes the stone at (0, 2) and is left with five stones on one liberty, the point it has just emptied
    ('snapback, white to move', fe.board(_SNAPBACK, white_to_move=True), [(0, 3, (1, 1, 5))]),
    ('the same point for black: four stones go', fe.board(_SNAPBACK), [(0, 3, (4, 4, 4))]),
    # two own chains of two, both on their last liberty, joined by a move that takes one stone: its point is the only liberty
    ('join two chains and capture', fe.board(_JOIN), [(1, 2, (1, 1, 5))]),
    ('captures in the corner and on the edge', fe.board(_EDGES), [(1, 0, (3, 1, 1)), (1, 3, (4, 1, 1)), (3, 3, (4, 0, 1))]),
    ('a capturing point marked in plane 3', fe.board(_EDGES, invalid=[(1, 3)]), [(1, 0, (3, 1, 1)), (1, 3, (0, 0, 0))]),
    # one stone taken by one stone that is left on one liberty: the ko shape, free and with its point marked in plane 3
    ('a ko capture', fe.board(_KO), [(1, 2, (1, 1, 1)), (0, 0, (1, 0, 3))]),
    ('the ko point marked in plane 3', fe.board(_KO, invalid=[(1, 2)]), [(1, 2, (0, 0, 0)), (0, 0, (1, 0, 3))]),
    ('the same board for white', fe.board(_EDGES, white_to_move=True), [(1, 0, (2, 0, 2)), (1, 3, (3, 0, 2)), (0, 5, (2, 0, 1))]),
    ('a suicide with plane 3 clear', fe.board(_SUICIDE), [(0, 0, (0, 0, 0)), (1, 1, (2, 0, 1))]),
    ('an ended game', fe.board(_EDGES, done=True), [(1, 0, (0, 0, 0)), (1, 3, (0, 0, 0)), (3, 3, (0, 0, 0))]),
    # 322 black stones in one chain with two empty rows below it
    ('a chain of more than 255 stones played into', fe.board(_full19(17)), [(0, 0, (19, 0, 323)), (17, 0, (20, 0, 323)),
                                                                           (18, 18, (2, 0, 1))]),
    # the same chain shut in by a white row: (0, 0) is its last liberty
    ('a capture of more than 255 stones', fe.board(_full19(17, white_row=17), white_to_move=True), [(0, 0, (2, 322, 1))]),
    ('its last liberty filled by the chain itself', fe.board(_full19(17, white_row=17)), [(0, 0, (0, 0, 0)), (18, 0, (1, 0, 1))]),
)


def crafted_by_size():
    """{N: (names, states uint8 [.., 6, N, N])} of CRAFTED."""
    out = {}
    for name, s, _ in CRAFTED:
        out.setdefault(s.shape[-1], ([], []))
        out[s.shape[-1]][0].append(name)
        out[s.shape[-1]][1].append(s)
    return {N: (names, np.stack(states)) for N, (names, states) in out.items()}
