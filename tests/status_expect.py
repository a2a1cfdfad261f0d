"""Stone status and the final score from playout ownership (gg_batch_status, gogame.batch_stone_status, batch_final_score) as
their definition says them - test infrastructure, CPU only, NumPy, SciPy and Python integers.

own int32 [2, N, N]: in how many of K playouts a point ended in black's (0) / white's (1) area.  A CHAIN is a component
(4-neighbourhood, scipy.ndimage.label) of the stones of one colour c; D = the sum of own[1 - c] over its stones, A = that of
own[c], n = its size:
    dead       iff D den >= num K n
    else alive iff A den >= num K n
    else unsettled
in Python integers.  The dead chains of both colours are taken off and tests/area_expect.py scores what remains.  From side's
view (0 black, 1 white; None: the state's turn plane):
    planes 0 / 1 / 2   own stones whose chain is alive / dead / unsettled
    planes 3 / 4 / 5   the opponent's
    planes 6 / 7 / 8   own area / opponent's area / neutral, after removal
    counts             own area, opponent's area, own dead stones, opponent's dead stones

generated(states, K, num, den): ownership counts that put the chains of given boards, in turn, exactly on each inequality, one
count below it, and well inside each status, with uneven per-stone values and with values on the empty points and the
neighbouring stones that would flip a chain if they were summed in.  large_case(): one chain of 360 stones at K = 2^20."""
import functools
from types import SimpleNamespace

import numpy as np
from scipy import ndimage

import area_expect as ae

NAMES = ('own_alive', 'own_dead', 'own_unsettled', 'opp_alive', 'opp_dead', 'opp_unsettled', 'own_area', 'opp_area', 'neutral')
PLANES = 9
WHITE_VIEW = (3, 4, 5, 0, 1, 2, 7, 6, 8)     # the planes of white's view as planes of black's; the counts: (1, 0, 3, 2)
THRESHOLDS = ((2, 3), (1, 1), (513, 1024))
PLAYOUTS = {(2, 3): 24, (1, 1): 8, (513, 1024): 2048}     # K, a multiple of den: equality is reachable
KINDS = ('dead_eq', 'dead_below', 'alive_eq', 'alive_below', 'dead', 'alive', 'unsettled')


def chains(state):
    """[(colour, bool [N, N])] of one state [6, N, N]: black's chains in label order, then white's."""
    out = []
    for c in (0, 1):
        labels, n = ndimage.label(state[c] != 0)          # (the 4-neighbourhood is the default structure)
        out += [(c, labels == k) for k in range(1, n + 1)]
    return out


def verdict(D, A, n, K, num, den):
    """'dead' / 'alive' / 'unsettled' of a chain of n stones with the sums D and A: Python integers throughout."""
    D, A, n, K, num, den = int(D), int(A), int(n), int(K), int(num), int(den)
    if D * den >= num * K * n:
        return 'dead'
    return 'alive' if A * den >= num * K * n else 'unsettled'


def vote(state, own, K, num, den):
    """(dead, alive) bool [2, N, N] each: per colour, the stones whose chain is dead / alive."""
    N = state.shape[-1]
    dead, alive = np.zeros((2, N, N), bool), np.zeros((2, N, N), bool)
    for c, m in chains(state):
        D = sum(int(v) for v in own[1 - c][m])
        A = sum(int(v) for v in own[c][m])
        v = verdict(D, A, int(m.sum()), K, num, den)
        if v == 'dead':
            dead[c] |= m
        elif v == 'alive':
            alive[c] |= m
    return dead, alive


def status_planes(state, own, K, num, den, side=None):
    """(uint8 [9, N, N], int32 [4]) of one state [6, N, N] and its own [2, N, N]."""
    dead, alive = vote(state, own, K, num, den)
    stones = np.stack([state[0] != 0, state[1] != 0])
    rest = np.array(state, np.uint8, copy=True)
    rest[0], rest[1] = stones[0] & ~dead[0], stones[1] & ~dead[1]
    white = bool(state[2, 0, 0]) if side is None else bool(side)
    area = ae.area_planes(rest, 1 if white else 0)
    me, op = (1, 0) if white else (0, 1)
    planes = np.stack([alive[me], dead[me], stones[me] & ~alive[me] & ~dead[me], alive[op], dead[op],
                       stones[op] & ~alive[op] & ~dead[op], area[0] != 0, area[1] != 0, area[2] != 0]).astype(np.uint8)
    return planes, np.array([area[0].sum(), area[1].sum(), dead[me].sum(), dead[op].sum()], np.int32)


def batch_status(states, own, K, num, den, side=None):
    """(uint8 [B, 9, N, N], int32 [B, 4]); side: None, one flag for all boards, or B flags."""
    states, own = np.asarray(states), np.asarray(own)
    B, N = len(states), states.shape[-1]
    sides = [None] * B if side is None else np.broadcast_to(np.asarray(side), (B,))
    if not B:
        return np.zeros((0, PLANES, N, N), np.uint8), np.zeros((0, 4), np.int32)
    res = [status_planes(s, o, K, num, den, v) for s, o, v in zip(states, own, sides)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def white_view(planes, counts):
    """Black's view of a result as white's: a permutation of the planes and of the counts."""
    return planes[..., WHITE_VIEW, :, :], counts[..., (1, 0, 3, 2)]


def final_score(states, own, K, num=2, den=3, komi=0.0):
    """dict of the fields of gogame.FinalScore (without its playouts) from the roots and the ownership of their playouts."""
    planes, counts = batch_status(states, own, K, num, den, side=0)
    margin = (counts[:, 0] - counts[:, 1]).astype(np.int32)
    return {'black_area': counts[:, 0], 'white_area': counts[:, 1], 'margin': margin, 'winner': np.sign(margin.astype(np.float64) - komi),
            'owner': planes[:, 6].astype(np.int8) - planes[:, 7].astype(np.int8), 'dead': planes[:, 1] | planes[:, 4],
            'unsettled': planes[:, 2] | planes[:, 5]}


def without_dead(states, dead):
    """The boards with the stones of `dead` (uint8 [B, N, N]) taken off."""
    out = np.array(states, np.uint8, copy=True)
    out[:, 0] &= 1 - dead
    out[:, 1] &= 1 - dead
    return out


# ---------------------------------------------------------------- generated ownership counts
def spread(total, caps, rng):
    """Integers v[i] in [0, caps[i]] that sum to `total`, drawn one after the other in a random order: uneven on purpose."""
    caps = [int(c) for c in caps]
    assert 0 <= total <= sum(caps), (total, caps)
    v = [0] * len(caps)
    order = rng.permutation(len(caps))
    left = sum(caps)
    for i in order:
        left -= caps[i]
        lo, hi = max(0, total - left), min(caps[i], total)
        v[i] = int(rng.integers(lo, hi + 1))
        total -= v[i]
    assert total == 0
    return v


def sums_of(kind, n, K, num, den, rng):
    """(D, A) of a chain of n stones for one of KINDS; K a multiple of den, eq = num K n / den the count on the inequality."""
    assert K % den == 0
    eq, top = num * (K // den) * n, K * n
    pick = lambda lo, hi: int(rng.integers(lo, hi + 1))
    if kind == 'dead_eq':
        return eq, top - eq                                 # D on the inequality, A as large as the contract allows
    if kind == 'dead_below':
        return eq - 1, min(top - (eq - 1), eq - 1)          # one count below: not dead - and A one below (or the rest): unsettled
    if kind == 'alive_eq':
        return min(top - eq, eq - 1), eq                    # A on the inequality, D as large as it can be without being dead
    if kind == 'alive_below':
        return min(top - (eq - 1), eq - 1), eq - 1
    if kind == 'dead':
        D = pick(eq, top)
        return D, pick(0, top - D)
    if kind == 'alive':
        A = pick(eq, top)
        return pick(0, min(top - A, eq - 1)), A
    D = pick(0, eq - 1)
    return D, pick(0, min(eq - 1, top - D))


def generated(states, K, num, den, seed=0):
    """own int32 [B, 2, N, N] for the boards, and info: one (board, colour, mask, kind, D, A) per chain.  The chains of a colour
    take KINDS in turn over the whole batch (black starts at KINDS[0], white at KINDS[3]).  Every empty point holds
    (K // 2, K - K // 2): either count, summed into a neighbouring chain that is one count below an inequality, would
    lift it over."""
    states = np.asarray(states)
    B, N = len(states), states.shape[-1]
    rng = np.random.default_rng([seed, N, K, num, den])
    own = np.zeros((B, 2, N, N), np.int32)
    own[:, 0], own[:, 1] = K // 2, K - K // 2
    info, turn = [], [0, 3]
    for b in range(B):
        for c, m in chains(states[b]):
            kind = KINDS[turn[c] % len(KINDS)]
            turn[c] += 1
            n = int(m.sum())
            D, A = sums_of(kind, n, K, num, den, rng)
            d = spread(D, [K] * n, rng)
            a = spread(A, [K - x for x in d], rng)
            own[b, 1 - c][m] = d
            own[b, c][m] = a
            info.append((b, c, m, kind, D, A))
    assert not B or (own.min() >= 0 and (own.sum(axis=1) <= K).all())
    return own, info


@functools.lru_cache(maxsize=None)
def case(N, kind, threshold=(2, 3)):
    """The expectation of plane_cases.case(N, kind) (kind 'corridor': of area_expect.corridor_boards(N)) with generated
    ownership counts, computed once: .states, .own, .K, .num, .den, .info, .black / .counts_black (side 0), .white /
    .counts_white (side 1), .planes / .counts (side None).  Read only."""
    import plane_cases as pc
    s = ae.corridor_boards(N).states if kind == 'corridor' else pc.case(N, kind).states
    num, den = threshold
    K = PLAYOUTS[threshold]
    own, info = generated(s, K, num, den, seed=len(kind))
    c = SimpleNamespace(N=N, kind=kind, states=s, own=own, K=K, num=num, den=den, info=info)
    c.black, c.counts_black = batch_status(s, own, K, num, den, side=0)
    c.white, c.counts_white = white_view(c.black, c.counts_black)
    white = (s[:, 2, 0, 0] != 0) if len(s) else np.zeros(0, bool)
    c.planes = np.where(white[:, None, None, None], c.white, c.black)
    c.counts = np.where(white[:, None], c.counts_white, c.counts_black)
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---------------------------------------------------------------- the large-value case
LARGE = dict(N=19, K=1 << 20, den=1024, stones=360)


@functools.lru_cache(maxsize=None)
def large_case(num):
    """Four 19x19 boards with ONE chain of 360 stones each (every point but (0, 0)) at K = 2^20, den = 1024: black's chain with D
    on the inequality and one count below it, then white's chain alike.  A is what the contract leaves.  num = 1024: every
    stone holds the full count (one of them K - 1 in the second form) and num K n is a multiple of 2^32; num = 1000: the
    per-stone values differ.  -> .states, .own, .K, .num, .den, .sums [(D, A)], .black, .counts_black."""
    N, K, den, n = (LARGE[k] for k in ('N', 'K', 'den', 'stones'))
    rng = np.random.default_rng([19, num])
    states = np.zeros((4, 6, N, N), np.uint8)
    own = np.zeros((4, 2, N, N), np.int32)
    own[:, 0, 0, 0], own[:, 1, 0, 0] = K // 2, K - K // 2          # the empty point: never read
    sums = []
    for i in range(4):
        c = i // 2
        states[i, c] = 1
        states[i, c, 0, 0] = 0
        states[i, 2] = i % 2
        m = states[i, c] != 0
        assert m.sum() == n
        D = num * (K // den) * n - (i % 2)
        d = spread(D, [K] * n, rng)
        own[i, 1 - c][m] = d
        own[i, c][m] = [K - x for x in d]
        sums.append((D, K * n - D))
    c = SimpleNamespace(states=states, own=own, K=K, num=num, den=den, sums=sums)
    c.black, c.counts_black = batch_status(states, own, K, num, den, side=0)
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---------------------------------------------------------------- hand-made positions
CRAFTED_7 = ['..B.W..',
             '..B.W..',
             '.WB.WB.',
             '..B.W..',
             'BBB.WWW',
             '..B.W..',
             '.B.BW.W']        # black to move: the white stone at (2, 1) and the black stone at (2, 5) are dead
LONE_5 = ['.....',
          '.B...',
          '.....',
          '...W.',
          '.....']              # one lone stone of each colour: both unsettled


def crafted_roots():
    """(the 7x7 position, the 5x5 position), black to move, with their invalid-move planes."""
    import mc_policy_expect as mp
    return mp.board(CRAFTED_7), mp.board(LONE_5)
