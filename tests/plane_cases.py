"""The positions the plane kernels (features, group liberties, life, ladder and their oriented forms) are checked on at EVERY
board size from 2 to 19, and what is expected of them - test infrastructure, CPU only, NumPy and the expect modules only.
Two generators, both deterministic in (N, seed): policy_positions (games of the no_eye_fill policy from the empty board at
three depths) and random_boards (independently placed stones: many tiny chains, dense boards, chains that touch many others,
chains without a liberty - shapes no game reaches).  case() computes the definitional expectation of a set once per process."""
import functools
from types import SimpleNamespace

import numpy as np

import features_expect as fe
import ladder_expect as lad
import life_expect as life
import mc_expect as mc
import mc_policy_expect as mp
import symmetry_expect as se

SIZES = tuple(range(2, 20))
B = 21                       # one board in the last wave in both layouts: 5 x 4 + 1 and 10 x 2 + 1
SETS = ('policy', 'random', 'clean')
LADDER_SETS = ('policy', 'clean')      # the ladder contract is silent on a start position with zero-liberty chains
# Seed offsets per N, where a not-vacuous assertion of tests/test_plane_cases_host.py asks for other boards than offset 0 gives:
# at 4 and 5 no policy game of the 21 has ended after 3 N^2 / 2 plies; at 7 and 17 the deepest ladder of the random boards
# (11, 21) is not deeper than that of the policy positions (19, 24).
POLICY_SEED_OFFSET = {4: 100, 5: 100}
SEED_OFFSET = {7: 3, 17: 3}


def policy_positions(N, B=B, seed=500):
    """uint8 [B, 6, N, N]: positions of the no_eye_fill policy from the empty board (the CPU policy_rollout, auto_reset off),
    a third of the boards each after N^2 / 2, N^2 and 3 N^2 / 2 plies; generators mc.po_seed(seed + N, arange(B))."""
    cur, rng = np.zeros((B, 6, N, N), np.uint8), mc.po_seed(seed + N, np.arange(B))
    cuts = [0, B // 3, 2 * B // 3, B]
    out, done = np.zeros_like(cur), 0
    for i, depth in enumerate((N * N // 2, N * N, 3 * N * N // 2)):
        cur, rng, _, _ = mp.policy_rollout(cur, rng, depth - done, auto_reset=False)
        done = depth
        out[cuts[i]:cuts[i + 1]] = cur[cuts[i]:cuts[i + 1]]
    return out


def uniform(key, n):
    """n numbers in [0, 1): the first splitmix64 output of each of the generators mc.po_seed(key, 0 .. n - 1) - plain
    integer arithmetic, the same numbers on every NumPy."""
    z = mc.po_seed(key, np.arange(n))
    with np.errstate(over='ignore'):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) / float(2 ** 53)


def random_boards(N, B=B, seed=0, clean=False):
    """uint8 [B, 6, N, N] of independently placed stones: board b has density (b % 7 + 1) / 8, either colour at 1 / 2, and
    white to move for odd b; built with features_expect.board.  clean=False: plane 3 is the stones, chains without liberties
    stay.  clean=True: every chain that fe.group_liberties counts at 0 is removed (one pass, both colours at once: what is
    left has a liberty), and every third board gets one random empty point marked in plane 3 (invalid=): a possible root ko
    of the ladder query, an illegal point of the legal plane."""
    P = N * N
    out = []
    for b in range(B):
        u = uniform(((seed + SEED_OFFSET.get(N, 0)) << 16) | (N << 8) | b, 2 * P + 1)
        stone = (u[:P] < (b % 7 + 1) / 8).reshape(N, N)
        black = (u[P:2 * P] < 0.5).reshape(N, N)
        g = np.where(stone, np.where(black, 'X', 'O'), '.')
        invalid = []
        if clean:
            s = fe.board([''.join(r) for r in g])
            g[(fe.group_liberties(s) == 0) & stone] = '.'
            empty = np.argwhere(g == '.')
            if b % 3 == 0 and len(empty):
                invalid = [tuple(int(v) for v in empty[min(int(u[2 * P] * len(empty)), len(empty) - 1)])]
        out.append(fe.board([''.join(r) for r in g], white_to_move=bool(b % 2), invalid=invalid))
    return np.stack(out)


def states_of(N, kind):
    if kind == 'policy':
        return policy_positions(N, seed=500 + POLICY_SEED_OFFSET.get(N, 0))
    return random_boards(N, seed=7, clean=kind == 'clean')


@functools.lru_cache(maxsize=None)
def case(N, kind):
    """One of SETS at size N with its expectation, computed once: .states, .features [B, 16, N, N], .libs [B, N, N],
    .life [B, 4, N, N], .settled [B]; for LADDER_SETS also .ladder [B, 4, N, N], .aborted [B], .stats.  Read only."""
    s = states_of(N, kind)
    c = SimpleNamespace(N=N, kind=kind, states=s, features=fe.batch_features(s), libs=fe.batch_group_liberties(s),
                        life=life.batch_life(s))
    c.settled = life.settled_of(c.life)
    if kind in LADDER_SETS:
        c.ladder, c.aborted, c.stats = lad.batch_ladder(s, stats=True)
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def oriented_ladder(N, kind, orient):
    """(planes, aborted) of the set's positions TURNED into the views `orient` (a tuple of B ints), then searched."""
    planes, aborted = lad.oriented(case(N, kind).states, np.array(orient) & 7)
    planes.setflags(write=False)
    aborted.setflags(write=False)
    return planes, aborted


def turned(planes, orient):
    """Row b of planes [B, C, N, N] in view orient[b] & 7."""
    return se.orient_images(planes, np.asarray(orient) & 7)
