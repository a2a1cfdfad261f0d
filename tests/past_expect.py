"""The definition of the history input planes (gogame.batch_past_planes, PuctSearch(past=); include/gymgo_amd_past.h) in NumPy,
from a list of byte-plane states, oldest first - the last one is the current position:

    planes(seq, T, moves)        uint8 [2 T + (T - 1 if moves else 0), N, N] of seq[-1]
    turned(planes, o)            the planes in view o (plane_cases.turned: symmetry_expect's geometry)
    ring(pushed, H, N)           (rows int32 [H, 2, N], count) a StoneHistory entry holds after pushing `pushed`, oldest first

and the games the tests use: played on the CPU by the pinned oracle (oracle.c_oracle.batch_next_states) from seeded legal
moves with passes mixed in.  Game g of size N draws its board moves from a w x w window in one corner (w = 3 + g, at most N),
so that stones meet, chains form and are captured within a few dozen plies at every board size; the numbers come from
plane_cases.uniform: integer arithmetic, the same on every NumPy."""
import functools
from types import SimpleNamespace

import numpy as np

import plane_cases as pc

MAX_T = 8
GAMES = 4          # per board size
PLIES = 40         # per game, unless it ends earlier (two passes in a row: only when nothing else is legal)
LARGEST_RING = MAX_T + 2
SEED_OFFSET = {16: 1, 18: 1}    # per board size: the first seed whose games hold what tests/test_past_host.py asks of the set


def plane_count(T, moves):
    return 2 * T + (T - 1 if moves else 0)


def planes(seq, T, moves):
    """The definition.  seq: [K, 6, N, N] (or a list), oldest first, K >= 1; position t is seq[-1 - t], absent for t >= K."""
    seq = np.asarray(seq)
    N = seq.shape[-1]
    cur = seq[-1]
    me = 1 if cur[2, 0, 0] else 0               # the colour to move NOW: plane 0 black, plane 1 white
    out = np.zeros((plane_count(T, moves), N, N), np.uint8)
    occ = []
    for t in range(T):
        if t < len(seq):
            s = seq[-1 - t]
            out[2 * t] = s[me] != 0
            out[2 * t + 1] = s[1 - me] != 0
            occ.append((s[0] != 0) | (s[1] != 0))
        else:
            occ.append(None)
    if moves:
        for t in range(T - 1):
            if occ[t + 1] is not None:
                out[2 * T + t] = occ[t] & ~occ[t + 1]
    return out


def turned(p, o):
    """planes [P, N, N] in view o."""
    return pc.turned(np.asarray(p)[None], [o])[0]


def turned_seq(seq, o):
    """every position of the game in view o: [K, 6, N, N]."""
    seq = np.asarray(seq)
    return pc.turned(seq, np.full(len(seq), o))


def rows_of(state):
    """int32 [2, N]: the black rows, then the white rows, of a state [6, N, N] as bit masks, bit c = column c."""
    N = state.shape[-1]
    w = (1 << np.arange(N, dtype=np.int64))
    r = ((np.asarray(state[:2]) != 0).astype(np.int64) * w).sum(axis=-1)
    return r.astype(np.uint32).view(np.int32)


def ring(pushed, H, N):
    """(rows int32 [H, 2, N], count): an empty ring after the pushes `pushed` (states, oldest first)."""
    rows = np.zeros((H, 2, N), np.int32)
    for k, s in enumerate(pushed):
        rows[k % H] = rows_of(s)
    return rows, len(pushed)


def with_ring(seq, count, H):
    """What a board sees whose ring of capacity H has had `count` pushes: its own position and the last min(count, H) before
    it - seq cut to that."""
    keep = min(max(count, 0), H)
    return seq[len(seq) - 1 - keep:]


@functools.lru_cache(maxsize=None)
def games(N):
    """GAMES games of size N -> a list of SimpleNamespace(states uint8 [K + 1, 6, N, N], actions int [K]): states[k] is the
    position before actions[k], states[K] the last one.  Read only."""
    P = N * N
    cur = np.zeros((GAMES, 6, N, N), np.uint8)
    states, actions = [[cur[g].copy()] for g in range(GAMES)], [[] for _ in range(GAMES)]
    live = np.ones(GAMES, bool)
    last_pass = np.zeros(GAMES, bool)
    from oracle import c_oracle
    for ply in range(PLIES):
        u = pc.uniform(((77 + SEED_OFFSET.get(N, 0)) << 20) | (N << 12) | ply, 2 * GAMES)
        acts = np.full(GAMES, P, np.int64)
        for g in range(GAMES):
            if not live[g]:
                continue
            w = min(N, 3 + g)
            r0, c0 = ((0, 0), (N - w, 0), (0, N - w), (N - w, N - w))[g % 4]
            window = np.zeros((N, N), bool)
            window[r0:r0 + w, c0:c0 + w] = True
            legal = np.flatnonzero(((cur[g, 3] == 0) & window).ravel())
            if len(legal) and (last_pass[g] or u[2 * g] >= 1 / 8):
                acts[g] = legal[min(int(u[2 * g + 1] * len(legal)), len(legal) - 1)]
        nxt, status = c_oracle.batch_next_states(cur, acts)
        assert not status[live].any(), (N, ply, status)
        for g in range(GAMES):
            if live[g]:
                cur[g] = nxt[g]
                states[g].append(nxt[g].copy())
                actions[g].append(int(acts[g]))
                last_pass[g] = acts[g] == P
                live[g] = not nxt[g, 5, 0, 0]
    out = []
    for g in range(GAMES):
        s, a = np.stack(states[g]), np.array(actions[g], np.int64)
        s.setflags(write=False)
        a.setflags(write=False)
        out.append(SimpleNamespace(states=s, actions=a))
    return out


def samples(N, B, lead=0):
    """B (game, ply) pairs of games(N) at different plies of different games, every one with at least `lead` plies behind it
    where its game is long enough: -> [(g, k)], board b sits before move k of game g (k may be the game's last position)."""
    gs = games(N)
    out = []
    for b in range(B):
        g = b % GAMES
        K = len(gs[g].actions)
        k = (lead + 3 * b + b // GAMES) % (K + 1)
        out.append((g, k))
    return out
