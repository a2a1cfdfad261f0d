"""Expected ladder planes (gogame.batch_ladder, batch_ladder_tracked), written the slow definitional way: CPU only, NumPy
only, a set-based board, plain recursion, explicit node and depth counters.  Shares no code with the kernels or with oracle/.

TERMS.  Colours, chains and liberties as in features_expect; points are ordered row-major.  The PREY is a chain, the
DEFENDER its colour, the ATTACKER the other colour.  A search is a sequence of legal moves on a copy of the position:
captures as in the rules (the opponent chains next to the played stone that have no liberty left go first); a move is legal
when the point is empty, is not the current ko point and, after captures, the played stone's chain has a liberty; a move
that captures exactly one stone and whose own chain is then that single stone with exactly one liberty makes the captured
point the ko point for the next move only.  At the root the ko point of the position (plane 11 of the feature planes)
applies exactly when the first player of the search is the player to move.

D(pos, c): the defender moves, c has exactly one liberty L.  Options, in order: L; then the sole liberty of each attacker
chain adjacent to c that has exactly one liberty - distinct points, row-major, L skipped.  A legal option leaves the chain c'
that holds c's stones with n liberties: n >= 3 escapes, n <= 1 fails, n == 2 escapes iff A(pos', c') is false.  D is true
(captured) iff no option escapes; evaluation stops at the first escape.
A(pos, c): the attacker moves, c has exactly two liberties L1 < L2.  For each Li in order that is legal for the attacker,
the option works iff D(pos', c) is true.  A is true iff some option works; evaluation stops at the first.

BOUNDS.  Every entry into D or A counts one node and has a depth, the number of moves played on the copy.  A root query
that would enter a node at depth > 4 N, or a node beyond number 16 N, is ABORTED: "not captured" for an attacker query,
"escapes" for a defender query, whatever had been found.

ROOT QUERIES, one budget each.  For a chain c with exactly two liberties and each Li: work(c, Li) iff Li is legal for the
attacker and D of the resulting position (depth 1) is true; false if aborted.  For a chain c with exactly one liberty and
each option o of D: esc(c, o) iff o is legal and escapes (its A, if any, at depth 1); true if aborted.  laddered(c): some
work(c, Li) / no esc(c, o); chains with no or with three and more liberties never.

PLANES [4, N, N], mover-relative: own stones of laddered chains, opponent stones of laddered chains, the points Li with
work(c, Li) for an opponent two-liberty chain, the points o with esc(c, o) for an own one-liberty chain; the last two are
clear when the game is over.  aborted = min(aborted root queries, 255)."""
import sys

import numpy as np

import features_expect as fe
import symmetry_expect as se

PLANES = 4
NAMES = ('own_laddered', 'opp_laddered', 'ladder_capture', 'ladder_escape')


def max_depth(N):
    return 4 * N


def max_nodes(N):
    return 16 * N


class Aborted(Exception):
    pass


class Budget:
    def __init__(self, N):
        self.N, self.nodes, self.depth = N, 0, 0

    def enter(self, depth):
        if depth > max_depth(self.N) or self.nodes + 1 > max_nodes(self.N):
            raise Aborted()
        self.nodes += 1
        self.depth = max(self.depth, depth)


def chain_at(stones, p, N):
    """The chain of the stone at p in the set `stones` -> frozenset."""
    seen, todo = {p}, [p]
    while todo:
        y, x = todo.pop()
        for q in fe.neighbours(y, x, N):
            if q in stones and q not in seen:
                seen.add(q)
                todo.append(q)
    return frozenset(seen)


def liberties(chain, pos, N):
    """The empty points next to the chain -> a sorted list (row-major)."""
    occupied = pos[0] | pos[1]
    return sorted({q for (y, x) in chain for q in fe.neighbours(y, x, N) if q not in occupied})


def play(pos, colour, p, ko, N):
    """pos = (black, white) frozensets; colour 0 / 1 plays p -> (pos', ko') or None when the move is not legal."""
    if p in pos[0] or p in pos[1] or p in ko:
        return None
    me, op = set(pos[colour]) | {p}, set(pos[1 - colour])
    captured = set()
    for q in fe.neighbours(p[0], p[1], N):
        if q in op and q not in captured:
            ch = chain_at(op, q, N)
            if not any(e not in me and e not in op for (y, x) in ch for e in fe.neighbours(y, x, N)):
                captured |= ch
    op -= captured
    new = (frozenset(me), frozenset(op)) if colour == 0 else (frozenset(op), frozenset(me))
    own = chain_at(me, p, N)
    libs = liberties(own, new, N)
    if not libs:
        return None
    return new, (frozenset(captured) if len(captured) == 1 and len(own) == 1 and len(libs) == 1 else frozenset())


def defender_options(pos, seed, defender, N):
    """The options of D for the prey that holds `seed`: its liberty, then the capturing points."""
    prey = chain_at(pos[defender], seed, N)
    libs = liberties(prey, pos, N)
    assert len(libs) == 1, libs
    caps = set()
    for (y, x) in prey:
        for q in fe.neighbours(y, x, N):
            if q in pos[1 - defender]:
                l2 = liberties(chain_at(pos[1 - defender], q, N), pos, N)
                if len(l2) == 1:
                    caps.add(l2[0])
    return libs + sorted(caps - set(libs))


def option_escapes(budget, pos, ko, seed, defender, o, depth):
    """The defender's option o at a node of depth `depth`."""
    N = budget.N
    res = play(pos, defender, o, ko, N)
    if res is None:
        return False
    pos2, ko2 = res
    n = len(liberties(chain_at(pos2[defender], seed, N), pos2, N))
    if n >= 3:
        return True
    if n <= 1:
        return False
    return not node_a(budget, pos2, ko2, seed, defender, depth + 1)


def node_d(budget, pos, ko, seed, defender, depth):
    budget.enter(depth)
    for o in defender_options(pos, seed, defender, budget.N):
        if option_escapes(budget, pos, ko, seed, defender, o, depth):
            return False
    return True


def node_a(budget, pos, ko, seed, defender, depth):
    budget.enter(depth)
    N = budget.N
    libs = liberties(chain_at(pos[defender], seed, N), pos, N)
    assert len(libs) == 2, libs
    for p in libs:
        res = play(pos, 1 - defender, p, ko, N)
        if res is not None and node_d(budget, res[0], res[1], seed, defender, depth + 1):
            return True
    return False


def ladder(state, stats=False):
    """uint8 [4, N, N] and the aborted count of one state [6, N, N]; with stats=True also a dict: queries, nodes (of all
    queries), depth (the deepest node of any query), aborts (not saturated), free (two-liberty chains that are not laddered),
    laddered (chains, per colour: black, white)."""
    state = np.asarray(state)
    N = state.shape[-1]
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    pts = lambda plane: frozenset((int(y), int(x)) for y, x in zip(*np.nonzero(plane)))
    pos = (pts(state[0]), pts(state[1]))
    mover = 1 if state[2, 0, 0] else 0
    done = bool(state[5, 0, 0])
    ko_root = pts(fe.features(state)[11])
    out = np.zeros((PLANES, N, N), np.uint8)
    st = dict(queries=0, nodes=0, depth=0, aborts=0, free=0, laddered=[0, 0])
    seen = set()
    for y in range(N):
        for x in range(N):
            p = (y, x)
            colour = 0 if p in pos[0] else 1 if p in pos[1] else -1
            if colour < 0 or p in seen:
                continue
            chain = chain_at(pos[colour], p, N)
            seen |= chain
            libs = liberties(chain, pos, N)
            if len(libs) == 2:       # attacker queries: the attacker moves first
                ko = ko_root if 1 - colour == mover else frozenset()
                works = []
                for li in libs:
                    budget = Budget(N)
                    st['queries'] += 1
                    try:
                        res = play(pos, 1 - colour, li, ko, N)
                        w = res is not None and node_d(budget, res[0], res[1], p, colour, 1)
                    except Aborted:
                        w = False
                        st['aborts'] += 1
                    st['nodes'] += budget.nodes
                    st['depth'] = max(st['depth'], budget.depth)
                    if w:
                        works.append(li)
                laddered = bool(works)
                st['free'] += not laddered
                if colour != mover and not done:
                    for q in works:
                        out[2][q] = 1
            elif len(libs) == 1:     # defender queries: the defender moves first
                ko = ko_root if colour == mover else frozenset()
                escapes = []
                for o in defender_options(pos, p, colour, N):
                    budget = Budget(N)
                    st['queries'] += 1
                    try:
                        e = option_escapes(budget, pos, ko, p, colour, o, 0)
                    except Aborted:
                        e = True
                        st['aborts'] += 1
                    st['nodes'] += budget.nodes
                    st['depth'] = max(st['depth'], budget.depth)
                    if e:
                        escapes.append(o)
                laddered = not escapes
                if colour == mover and not done:
                    for q in escapes:
                        out[3][q] = 1
            else:
                continue
            if laddered:
                st['laddered'][colour] += 1
                for q in chain:
                    out[0 if colour == mover else 1][q] = 1
    aborted = min(st['aborts'], 255)
    return (out, aborted, st) if stats else (out, aborted)


def batch_ladder(states, stats=False):
    """-> (planes uint8 [B, 4, N, N], aborted uint8 [B]) (and the list of stats)."""
    states = np.asarray(states)
    if not len(states):
        res = (np.zeros((0, PLANES) + states.shape[2:], np.uint8), np.zeros(0, np.uint8))
        return res + ([],) if stats else res
    rows = [ladder(s, stats=True) for s in states]
    res = (np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.uint8))
    return res + ([r[2] for r in rows],) if stats else res


def oriented(states, orient):
    """The planes and aborted counts of the TURNED positions: row b of states in view orient[b] (symmetry_expect's
    orientations), turned first, then searched - the row-major tie-breaks are those of the view."""
    states = np.asarray(states)
    return batch_ladder(se.orient_images(states, np.asarray(orient)))


# ---------------------------------------------------------------- boards for the tests
def swap(rows):
    return [r.replace('X', 'x').replace('O', 'X').replace('x', 'O') for r in rows]


def pad(rows, N):
    """rows, filled up to N x N with empty points."""
    return [r + '.' * (N - len(r)) for r in rows] + ['.' * N] * (N - len(rows))


def staircase(N, breaker=False):
    """The textbook ladder: the white stone at (1, 1) has the two liberties (1, 2) and (2, 1), and either atari drives it down
    the diagonal into the far edge.  breaker: a white stone on the path, which the prey reaches with three liberties."""
    g = [['.'] * N for _ in range(N)]
    g[1][1] = 'O'
    g[0][1] = g[1][0] = 'X'
    g[2][0] = 'X'      # (1, 0) - (2, 0): the chain under the prey is not short of liberties itself
    if breaker:
        g[N - 3][N - 2] = 'O'
    return [''.join(r) for r in g]


LADDER9 = staircase(9)
BROKEN9 = staircase(9, True)
LADDER19 = staircase(19)

# the white pair (0, 2), (1, 2) has one liberty, (0, 1); extending there leaves one liberty, capturing the black pair in atari
# at (2, 3) leaves three
CAPTURE_SAVES = ['..OXO..',
                 '.XOXO..',
                 '..X....',
                 '.......',
                 '.......',
                 '.......',
                 '.......']

# the white pair's only liberty (0, 0) is suicide, and no chaser is in atari
SUICIDE = ['.OX..',
           'XOX..',
           'XX...',
           '.....',
           '.....']

# white (2, 2) has the liberty (3, 2); extending leaves one liberty, capturing (1, 2) at (1, 1) leaves two - and makes (1, 2)
# the ko point, so that the attacker cannot take back there; with (1, 1) the ROOT ko point, white cannot capture at all
KO = ['XXOO...',
      'X.XOO..',
      'XXOX...',
      '.X.X...',
      '.......',
      '.......',
      '.......']

# found by search: one root query of the board runs into the node bound / into the depth bound
NODE_BOUND9 = ['.O..XO.XX', 'XOOX.O..X', 'XOOO...OX', 'O..OX..XO', '...OO.X.O', 'X..X..O.X', 'XO.XX..OX', 'X.O..O.X.', 'O.X...OXX']
NODE_BOUND7 = ['XXXX...', 'XO.X..O', '.......', 'X.X....', 'O.OXOXX', 'O.XO..X', 'OOO.XX.']
DEPTH_BOUND7 = ['.O..X.X', '.OOXO..', 'X.O....', '.XX...X', 'OOO..X.', 'O.O..OX', '..XX...']

# found by search as well: the one aborted query of the board has another answer with the bounds out of reach, so the
# conservative answer shows.  ATTACKER: an atari that works is not marked (DEPTH: white's at (0, 1), and black (0, 0) is still
# laddered by the atari at (1, 0); NODES: black's at (5, 4), and white (6, 4) is not laddered).  DEFENDER: a move that does
# not get the chain out is marked and the chain is not laddered (DEPTH: black (0, 0) and its extension (1, 0); NODES: white
# (0, 2) and the capture at (0, 3))
ABORT_DEPTH_ATTACKER = ['X......', '..O....', '....O.X', '.X....X', 'O......', 'O......', '..X.OOO']
ABORT_DEPTH_DEFENDER = ['XO.....', '..O....', '....O.X', '.X....X', 'O......', 'O......', '..X.OOO']
ABORT_NODES_ATTACKER = ['XXX....', 'XX..O.X', '....XXO', '.....O.', 'X...X..', '.......', '....OXO']
ABORT_NODES_DEFENDER = ['XXO....', '.OX....', '.X...X.', '.....XX', '..O..XO', '.......', '.......']


def forms(rows, **kw):
    """The position with black / white to move, and both again with the colours swapped."""
    return [fe.board(r, white_to_move=white, **kw) for r in (rows, swap(rows)) for white in (False, True)]


def crafted(N):
    """The crafted positions of an N x N board (2, 5, 7, 9 or 19) -> uint8 [.., 6, N, N]: the ladder that works FIRST (the
    tests index it), the broken one, an ended game, the empty board (9) and a full board (10), then the hand-worked and the
    searched boards of that size.  At 2 x 2 the two hand-made boards stand where the ladders do."""
    if N == 2:
        out = forms(['X.', '.O']) + forms(['XO', 'O.'])
        out += [fe.board(['X.', '.O'], done=True), fe.board(['..', '..']), fe.board(['XX', 'XX']), fe.board(['XO', 'XO'])]
        return np.stack(out)
    out = forms(staircase(N)) + forms(staircase(N, True))
    out += [fe.board(staircase(N), done=True), fe.board(['.' * N] * N), fe.board(['X' * N] * N),
            fe.board(['XO' * (N // 2) + 'X'] * N)]
    if N == 5:
        out += forms(SUICIDE) + forms(['XOXOX'] * 5)
    if N == 7:
        for rows in (CAPTURE_SAVES, KO, NODE_BOUND7, DEPTH_BOUND7, ABORT_DEPTH_ATTACKER, ABORT_DEPTH_DEFENDER,
                     ABORT_NODES_ATTACKER, ABORT_NODES_DEFENDER):
            out += forms(rows)
        out.append(fe.board(KO, white_to_move=True, invalid=[(1, 1)]))
    if N == 9:
        out += forms(NODE_BOUND9)
    return np.stack(out)
