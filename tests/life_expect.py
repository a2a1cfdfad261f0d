"""Expected pass-alive (Benson) life planes (gogame.batch_life, batch_life_tracked, batch_settled), written the slow
definitional way: CPU only, NumPy only, a breadth-first search per chain and per region, then Benson's two-step iteration
on Python sets.  Shares no code with the kernels or with oracle/.

For a colour X: S = its stones, O = the other colour's, E = the empty points.  CHAINS are the connected components of S,
REGIONS the connected components of the complement of S (E and O together).  A region is VITAL to a chain when it holds an
empty point and every empty point of it is adjacent to a stone of the chain; it BORDERS a chain when some point of it is.
A = all chains, Q = all regions; until neither changes: (1) drop from A every chain with fewer than two regions of Q vital
to it, (2) drop from Q every region that borders a chain of X not in A.  alive(X) = the stones of A, safe(X) = the points of
the regions of Q vital to at least one chain of A.  Planes, mover-relative: alive(own), alive(opponent), safe(own),
safe(opponent); settled = every point lies in some plane."""
from collections import deque

import numpy as np

import features_expect as fe
import symmetry_expect as se

PLANES = 4
NAMES = ('own_alive', 'opp_alive', 'own_safe', 'opp_safe')


def components(mask):
    """The connected components (orthogonal adjacency) of a bool [N, N] mask -> a list of frozensets of (y, x)."""
    N = mask.shape[0]
    seen = np.zeros((N, N), bool)
    out = []
    for y0 in range(N):
        for x0 in range(N):
            if not mask[y0, x0] or seen[y0, x0]:
                continue
            seen[y0, x0] = True
            todo, comp = deque([(y0, x0)]), []
            while todo:
                y, x = todo.popleft()
                comp.append((y, x))
                for ny, nx in fe.neighbours(y, x, N):
                    if mask[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        todo.append((ny, nx))
            out.append(frozenset(comp))
    return out


def benson(stones, other):
    """-> (alive bool [N, N], safe bool [N, N], iterations) of the colour with `stones` against `other` (bool [N, N]);
    iterations = the number of times step 1 dropped a chain."""
    N = stones.shape[0]
    empty = ~stones & ~other
    chains = components(stones)
    regions = components(~stones)
    around = lambda pts: {q for (y, x) in pts for q in fe.neighbours(y, x, N)}
    chain_nb = [around(c) for c in chains]                       # the points adjacent to a stone of the chain
    region_e = [{p for p in r if empty[p]} for r in regions]
    vital = [[bool(region_e[j]) and region_e[j] <= chain_nb[i] for j in range(len(regions))] for i in range(len(chains))]
    borders = [[bool(chain_nb[i] & regions[j]) for j in range(len(regions))] for i in range(len(chains))]
    A, Q = set(range(len(chains))), set(range(len(regions)))
    iterations = 0
    while True:
        A2 = {i for i in A if sum(1 for j in Q if vital[i][j]) >= 2}
        Q2 = {j for j in Q if not any(borders[i][j] for i in range(len(chains)) if i not in A2)}
        if A2 != A:
            iterations += 1
        if A2 == A and Q2 == Q:
            break
        A, Q = A2, Q2
    alive, safe = np.zeros((N, N), bool), np.zeros((N, N), bool)
    for i in A:
        for p in chains[i]:
            alive[p] = True
    for j in Q:
        if any(vital[i][j] for i in A):
            for p in regions[j]:
                safe[p] = True
    return alive, safe, iterations


def life(state):
    """uint8 [4, N, N] of one state [6, N, N]; only planes 0, 1 and 2 are read."""
    state = np.asarray(state)
    black, white = state[0] != 0, state[1] != 0
    ab, sb, _ = benson(black, white)
    aw, sw, _ = benson(white, black)
    if state[2, 0, 0]:
        return np.stack([aw, ab, sw, sb]).astype(np.uint8)
    return np.stack([ab, aw, sb, sw]).astype(np.uint8)


def iterations(state):
    """The larger of the two colours' numbers of iterations that dropped a chain."""
    state = np.asarray(state)
    black, white = state[0] != 0, state[1] != 0
    return max(benson(black, white)[2], benson(white, black)[2])


def batch_life(states):
    states = np.asarray(states)
    return np.stack([life(s) for s in states]) if len(states) else np.zeros((0, PLANES) + states.shape[2:], np.uint8)


def settled_of(planes):
    """uint8 [B] from planes [B, 4, N, N]: 1 iff every point lies in some plane."""
    planes = np.asarray(planes)
    return (planes != 0).any(axis=1).all(axis=(1, 2)).astype(np.uint8)


def settled(states):
    return settled_of(batch_life(states))


def oriented(planes, orient):
    """Row b of planes [B, 4, N, N] in view orient[b] (symmetry_expect's orientations)."""
    return se.orient_images(np.asarray(planes), orient)


# ---------------------------------------------------------------- boards for the tests
def swap(rows):
    return [r.replace('X', 'x').replace('O', 'X').replace('x', 'O') for r in rows]


def cascade(N, filled):
    """Black chains c1 .. cL stacked from the first row down (L = (N - 2) // 3 + 1: 6 on 19x19, 3 on 9x9).  c1 is rows 0 - 1
    with two one-point eyes of its own at (0, 0) and (0, 2).  c(i+1) is two full rows with ONE one-point eye of its own, the
    second point from the end of its upper row, closed from above by two stones (teeth) that stand in the row between the
    chains; the rest of that row and the three points of ci's lower row over the teeth are white stones, but for one empty
    point beside the teeth.  That region touches ci (its white stones do) and its only empty point touches c(i+1) alone: it
    is vital to c(i+1) and to nothing else, and it falls out of Q when ci dies.  So every chain has exactly two vital regions
    and all are alive (the open area below the last chain holds a point that touches no stone); with filled=True, (0, 2) holds a black stone, c1 keeps one eye, and the chains die one per iteration."""
    g = [['.'] * N for _ in range(N)]
    L = (N - 2) // 3 + 1
    for x in range(N):
        g[0][x] = g[1][x] = 'X'
    g[0][0] = '.'
    g[0][2] = 'X' if filled else '.'
    for i in range(1, L):
        top = 3 * i                      # rows top, top + 1: the chain; row top - 1: the row between
        teeth, beside = ((N - 1, N - 2), N - 3) if i % 2 == 1 else ((0, 1), 2)
        for x in range(N):
            g[top][x] = g[top + 1][x] = 'X'
            g[top - 1][x] = 'O'
        for x in teeth + (beside,):
            g[top - 2][x] = 'O'          # the lower row of the chain above, over the teeth
            g[top - 1][x] = 'X'
        g[top - 1][beside] = '.'
        g[top][teeth[1]] = '.'
    if 3 * (L - 1) + 1 == N - 2:         # one row left below the last chain: open its far corner, or that row would be vital to it
        g[N - 2][N - 1 if (L - 1) % 2 == 0 else 0] = '.'
    return [''.join(r) for r in g], L


def crafted(N):
    """The cascade boards at size N (9 or 19), alive and dying, each with black and with white to move and with the colours
    swapped -> uint8 [8, 6, N, N]."""
    out = []
    for filled in (False, True):
        rows, _ = cascade(N, filled)
        for r in (rows, swap(rows)):
            for white in (False, True):
                out.append(fe.board(r, white_to_move=white))
    return np.stack(out)


SMALL = (
    # a corner group with two one-point eyes / with one / two chains sharing their only two eyes / a false eye at the edge
    ['.X.X.', 'XXXX.', '.....', '.....', '.....'],
    ['.XX..', 'XXX..', '.....', '.....', '.....'],
    ['.X.X.', 'XX.XX', '..X..', 'XXXXX', '.....'],
    ['.X.X.', 'X.XX.', '.X...', '.....', '.....'],
    # an eye holding an opponent stone / a bent three-point eye / a 2x2 eye / a large eye with an untouched interior point
    ['.OX..', 'XXX.X', '..XXX', '.....', '.....'],
    ['..X.X', '.XXXX', 'XX...', '.....', '.....'],
    ['..X.X', '..XXX', 'XXX..', '.....', '.....'],
    ['...X.', '...XX', '...X.', 'XXXX.', '.....'],
)


def small_boards():
    """SMALL, each with black and white to move and with the colours swapped, then the empty board, one stone and a full
    board -> uint8 [.., 6, 5, 5]."""
    out = []
    for rows in SMALL:
        for r in (rows, swap(rows)):
            for white in (False, True):
                out.append(fe.board(r, white_to_move=white))
    for rows in (['.....'] * 5, ['.....', '.....', '..X..', '.....', '.....'], ['XXXXX', 'XXOXX', 'XOOOX', 'XXOXX', 'XXXXX']):
        for white in (False, True):
            out.append(fe.board(rows, white_to_move=white))
    return np.stack(out)
