"""Expected position hashes, move hashes and repeat masks (gogame.batch_hash, batch_move_hashes, batch_superko_moves and their
tracked forms), written the slow definitional way: CPU only, the keys from Python integers, the hash from a loop over the
stones, the child by playing the stone on a copy of the board and removing the opponent chains without a liberty
(breadth-first, outcome_expect.chain), the repeat mask by a set lookup - point by point from include/gymgo_amd.h.  Shares no
code with the kernels, gogame.zobrist_keys or oracle/.  Also the game set of the tests: uniform games without voluntary
passes on 2x2 and 3x3, the boards on which positions repeat."""
import functools
from types import SimpleNamespace

import numpy as np

import features_expect as fe
import outcome_expect as oe

SEED = 0x676F2D6861736821
MASK = (1 << 64) - 1


def _keys():
    x, out = SEED, []
    for _ in range(2 * 19 * 19):
        x = (x + 0x9E3779B97F4A7C15) & MASK
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        out.append(z ^ (z >> 31))
    return out


KEYS = _keys()      # 722 Python integers in [0, 2^64)


def key(c, y, x):
    """colour c (0 black, 1 white) at row y, column x: independent of the board size"""
    return KEYS[c * 361 + y * 19 + x]


def signed(v):
    """an unsigned 64-bit pattern as the int64 the device returns"""
    return v - (1 << 64) if v >= (1 << 63) else v


def hash_stones(black, white):
    """the XOR of the keys over the stones of two [N, N] planes, as a signed Python integer"""
    h = 0
    for y, x in np.argwhere(np.asarray(black) != 0):
        h ^= key(0, int(y), int(x))
    for y, x in np.argwhere(np.asarray(white) != 0):
        h ^= key(1, int(y), int(x))
    return signed(h)


def hash_of(state):
    s = np.asarray(state)
    return hash_stones(s[0], s[1])


def child(state, y, x):
    """The mover's stone on the empty point (y, x), opponent chains without a liberty removed (the played chain stays whatever
    its liberties) -> (black [N, N] bool, white [N, N] bool, stones captured, chains captured)."""
    s = np.asarray(state)
    N = s.shape[-1]
    white = bool(s[2, 0, 0])
    own, opp = (s[1], s[0]) if white else (s[0], s[1])
    grid = np.where(own != 0, oe.OWN, np.where(opp != 0, oe.OPP, oe.EMPTY))
    assert grid[y, x] == oe.EMPTY
    grid[y, x] = oe.OWN
    captured, chains = set(), 0
    for q in fe.neighbours(y, x, N):
        if grid[q] == oe.OPP and q not in captured:
            stones, libs = oe.chain(grid, *q)
            if not libs:
                captured |= stones
                chains += 1
    for q in captured:
        grid[q] = oe.EMPTY
    mine, theirs = grid == oe.OWN, grid == oe.OPP
    return (theirs, mine, len(captured), chains) if white else (mine, theirs, len(captured), chains)


def move_hashes(state):
    """int64 [N*N + 1]: the child's hash at every candidate, the board's own at the pass and everywhere else"""
    s = np.asarray(state)
    N = s.shape[-1]
    out = np.full(N * N + 1, hash_of(s), np.int64)
    for y, x in np.argwhere(oe.candidates(s)):
        b, w, _, _ = child(s, int(y), int(x))
        out[y * N + x] = hash_stones(b, w)
    return out


def batch_hash(states):
    return np.array([hash_of(s) for s in np.asarray(states)], np.int64)


def batch_move_hashes(states):
    states = np.asarray(states)
    N = states.shape[-1]
    return np.stack([move_hashes(s) for s in states]) if len(states) else np.zeros((0, N * N + 1), np.int64)


def repeat_mask(state, hashes, history, count):
    """uint8 [N*N + 1]: candidate points whose move hash is among the first min(max(count, 0), H) entries of history [H]"""
    s = np.asarray(state)
    N = s.shape[-1]
    valid = {int(v) for v in np.asarray(history)[:min(max(int(count), 0), len(history))]}
    out = np.zeros(N * N + 1, np.uint8)
    for y, x in np.argwhere(oe.candidates(s)):
        out[y * N + x] = int(hashes[y * N + x]) in valid
    return out


def batch_repeat(states, hashes, history, count):
    return np.stack([repeat_mask(s, h, hist, c) for s, h, hist, c in zip(states, hashes, history, count)])


def rows_of(repeat, N):
    """the repeat points [B, N*N + 1] as row masks int32 [B, N]: bit x of row y"""
    pts = np.asarray(repeat)[:, :N * N].reshape(-1, N, N).astype(np.int64)
    return (pts << np.arange(N)[None, None, :]).sum(axis=2).astype(np.uint32).view(np.int32)


@functools.lru_cache(maxsize=None)
def case(N, kind):
    """The set `kind` of tests/plane_cases.py at size N with its expectation, computed once: .states, .hashes int64 [B],
    .moves int64 [B, N*N + 1].  Read only."""
    import plane_cases as pc
    s = pc.states_of(N, kind)
    c = SimpleNamespace(N=N, kind=kind, states=s, hashes=batch_hash(s), moves=batch_move_hashes(s))
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---------------------------------------------------------------- the game set
GAMES, PLIES = 64, 40
GAME_SEEDS = {2: 11, 3: 11}     # np.random.RandomState seeds of the draws, per board size


def position_key(black, white):
    return np.asarray(black, bool).tobytes() + np.asarray(white, bool).tobytes()


@functools.lru_cache(maxsize=None)
def games(N):
    """GAMES uniform games of PLIES plies from the empty board, played by the C restatement: every ply draws uniformly among the
    points plane 3 allows and passes only when there is none; a game that has ended stays where it is.  -> .states uint8
    [GAMES, PLIES, 6, N, N] (the position before each ply), .actions int32 [GAMES, PLIES] (-1 once the game has ended).
    Read only."""
    from oracle import c_oracle
    rs = np.random.RandomState(GAME_SEEDS[N])
    cur = np.zeros((GAMES, 6, N, N), np.uint8)
    states = np.zeros((GAMES, PLIES, 6, N, N), np.uint8)
    actions = np.full((GAMES, PLIES), -1, np.int32)
    for t in range(PLIES):
        states[:, t] = cur
        live = np.flatnonzero(cur[:, 5, 0, 0] == 0)
        if not len(live):
            continue
        acts = []
        for g in live:
            free = np.flatnonzero(cur[g, 3].reshape(-1) == 0)
            acts.append(int(free[rs.randint(len(free))]) if len(free) else N * N)
        nxt, status = c_oracle.batch_next_states(cur[live], np.array(acts, np.int32))
        assert not status.any()
        cur = cur.copy()
        cur[live] = nxt
        actions[live, t] = acts
    states.setflags(write=False)
    actions.setflags(write=False)
    return SimpleNamespace(N=N, states=states, actions=actions)


def recreating_moves(states):
    """For the positions [T, 6, N, N] of ONE game in order: the (t, action) pairs where the board move `action`, a candidate of
    position t, makes a position (compared stone by stone, not by hash) that the game has been in at some ply <= t."""
    seen, out = set(), []
    N = states.shape[-1]
    for t, s in enumerate(states):
        seen.add(position_key(s[0], s[1]))
        for y, x in np.argwhere(oe.candidates(s)):
            b, w, _, _ = child(s, int(y), int(x))
            if position_key(b, w) in seen:
                out.append((t, int(y) * N + int(x)))
    return out


def game_histories(g):
    """All (game, ply) pairs of a game set as one batch: states [G*T, 6, N, N], history int64 [G*T, T + 1] (the hashes of the
    game's positions 0 .. ply, zero beyond), count int32 [G*T] = ply + 1."""
    G, T = g.states.shape[:2]
    hashes = np.array([[hash_of(s) for s in game] for game in g.states], np.int64)     # [G, T]
    hist = np.zeros((G, T, T + 1), np.int64)
    for t in range(T):
        hist[:, t, :t + 1] = hashes[:, :t + 1]
    count = np.tile(np.arange(1, T + 1, dtype=np.int32), G)
    return g.states.reshape((G * T,) + g.states.shape[2:]), hist.reshape(G * T, T + 1), count
