"""Expected results of the move priors and of the RAVE search with priors (gogame.batch_move_priors, batch_uct(rave_equiv=...,
prior=...); include/gymgo_amd_prior.h) - test infrastructure, CPU only, built on tests/mc_tactics_expect.py (C, E, F),
tests/mc_pattern_expect.py (P, L) and tests/mc_amaf_expect.py (the RAVE tree and its playouts).

The rule: for a legal point p of a board, pair(p) = even + [p in C] capture + [p in E] escape + [p in P] pattern + [p in L] local
+ [p in X] eye_fill, X = the legal points that are not in F; (0, 0) for every other point.  A node of the tree starts with
(visits, 2 wins) of its board's pairs ADDED to its (n~, s~): the root at construction with the caller's previous action, a new
node when select creates it, with the expanded action as its previous action (the pass: none).  The cases the device tests run
are functions of their arguments alone and cached, so tests/test_prior_host.py (their premises) and tests/test_gpu_prior.py (the
comparison) share one computation."""
import collections
import functools
import math

import numpy as np

import mc_amaf_expect as ma
import mc_cases as cs
import mc_expect as mc
import mc_pattern_expect as mq
import mc_policy_expect as mp
import mc_tactics_expect as mt

TERMS = ('even', 'capture', 'escape', 'pattern', 'local', 'eye_fill')
Prior = collections.namedtuple('Prior', TERMS)
DEFAULT = Prior((8, 4), (8, 8), (8, 8), (4, 4), (8, 8), (16, 0))          # gogame.UCT_PRIOR (tests/test_prior_host.py holds them together)
LOPSIDED = Prior((1, 0), (30, 29), (5, 1), (3, 2), (12, 3), (40, 0))
ZERO = Prior(*[(0, 0)] * 6)


def prior_sets(states, last):
    """-> the six sets of TERMS, bool [B, N, N] each: valid, C, E, P and valid, L, X."""
    states = np.asarray(states)
    C, E, F = mt.tiers(states)
    P, L = mq.pattern_sets(states, last)
    ended = states[:, 5, 0, 0] != 0
    valid = (states[:, 3] == 0) & ~ended[:, None, None]
    return valid, C, E, P & valid, L, valid & ~F


def prior_pairs(states, last, weights):
    """-> int64 [B, N*N, 2]: (visits, 2 wins) of every point of every board.  last: None, or the previous action of every board
    (anything that is no point of the board: none); weights: six (visits, wins) pairs in the order of TERMS."""
    states = np.asarray(states)
    B, _, N, _ = states.shape
    sets = prior_sets(states, last)
    for s in sets[1:]:
        assert not (s & ~sets[0]).any()                      # every set lies inside valid
    out = np.zeros((B, N * N, 2), np.int64)
    for s, (v, w) in zip(sets, weights):
        assert 0 <= w <= v
        out[:, :, 0] += s.reshape(B, -1) * int(v)
        out[:, :, 1] += s.reshape(B, -1) * (2 * int(w))
    return out


class PriorTree(ma.RaveTree):
    def __init__(self, root, I, weights, last=None):
        super().__init__(root, I)
        self.weights = weights
        self.node_amaf[0] += prior_pairs(root[None], None if last is None else [last], weights)[0]
        self.first_expanded = None

    def select(self, K, c, L, k, fpu):
        y, board, new = super().select(K, c, L, k, fpu)
        if new:
            if self.first_expanded is None:
                self.first_expanded = int(self.action[y])
            self.node_amaf[y] += prior_pairs(board[None], [int(self.action[y])], self.weights)[0]
        return y, board, new


def expected_uct_prior(roots, I, K, weights, last_actions=None, **kw):
    """mc_amaf_expect.expected_uct_rave (and its keywords) on PriorTrees: -> dict of the outputs of batch_uct(rave_equiv=...,
    prior=weights, last_actions=..., tree=True) (NumPy), 'replayed' included, plus 'child' in 'tree', and for the premises 'first'
    (per root: the first expanded action, None for a root that expands nothing)."""
    roots = np.ascontiguousarray(roots, np.uint8)
    trees = [PriorTree(roots[r], I, weights, None if last_actions is None else int(last_actions[r])) for r in range(len(roots))]
    out = ma.expected_uct_rave(roots, I, K, trees=trees, **kw)
    out['tree']['child'] = np.stack([t.child for t in trees]).astype(np.int32)
    out['first'] = [t.first_expanded for t in trees]
    return out


# ---------------------------------------------------------------- the boards of the pairs test
SIZES = tuple(range(2, 20))


@functools.lru_cache(maxsize=None)
def pair_boards(N):
    """-> (states uint8 [B, 6, N, N], last int32 [B]): about 40 boards per size - mt.pool(N) (named roots with a ko root from N = 4 on
    and finished games, positions of random play, at 5x5 the hand-made capture and escape positions), at 5x5 also the hand-made
    pattern positions with their previous moves, at 19x19 the seam roots of both modules; the previous actions of the pool
    cycle over mq.last_cycle's."""
    states = [b for b in mt.pool(N)]
    last = list(mq.last_cycle(N, len(states)))
    if N == 5:
        for _, b, prev, _, _ in mq.crafted_positions():
            if b.shape[-1] == N:
                states.append(b)
                last.append(-1 if prev is None else prev[0] * N + prev[1])
    if N == 19:
        states += list(mt.seam_roots())
        last += [9 * 19 + 3, 10 * 19 + 7]
        sr, sl = mq.seam_roots()
        states += list(sr[:8])
        last += list(sl[:8])
    states, last = np.stack(states), np.array(last, np.int32)
    states.setflags(write=False)
    last.setflags(write=False)
    return states, last


def last_variants(N, B, real):
    """The four forms of `last` the pairs test runs: None, all -1, all the pass, real previous actions."""
    return (('none', None), ('minus_one', np.full(B, -1, np.int32)), ('pass', np.full(B, N * N, np.int32)), ('real', real))


def mixed_boards(B):
    """B boards of 9x9 for the grid-stride test: pair_boards(9) over and over with their previous actions."""
    st, la = pair_boards(9)
    i = np.arange(B) % len(st)
    return st[i], la[i]


# ---------------------------------------------------------------- the cases of the tree test
TREE_SIZES = ma.RAVE_SIZES
TREE_I, TREE_K, TREE_EQUIV, TREE_FPU, TREE_KOMI = ma.RAVE_I, ma.RAVE_K, ma.RAVE_EQUIV, 0.5, ma.RAVE_KOMI
TREE_CS = ma.RAVE_CS
# (c, prior, with last_actions): every value of each parameter with every value of the two others' at least once
TREE_VARIANTS = ((0.0, 'default', False), (math.sqrt(2), 'default', True), (0.0, 'lopsided', True), (math.sqrt(2), 'lopsided', False))
PRIORS = {'default': DEFAULT, 'lopsided': LOPSIDED, 'zero': ZERO}


def crafted_root(N):
    """A root with a capture for the mover: from 5x5 on mt.crafted_positions' capture_and_escape_apart in the top left corner (a
    white stone to take at (2, 3), a black one to save at (2, 0)); below, a white corner stone in atari."""
    if N >= 5:
        rows = ['.WB..', '.BW..', '.WB..']
        text = ['.' * N] + [r + '.' * (N - 5) for r in rows] + ['.' * N] * (N - 4)
    else:
        text = ['WB' + '.' * (N - 2)] + ['.' * N] * (N - 1)
    return mp.board(text)


@functools.lru_cache(maxsize=None)
def tree_roots(N):
    """-> (roots uint8 [5, 6, N, N], last_actions int32 [5]): ma.rave_roots(N) - a late root, a mid-game root, the empty board, a
    finished game - and crafted_root(N); the previous actions: a point, the pass, -1, a point, the white stone next to the capture."""
    roots = np.concatenate([ma.rave_roots(N), crafted_root(N)[None]])
    P = N * N
    last = np.array([P // 2, P, -1, 0, (2 * N + 2) if N >= 5 else 0], np.int32)
    roots.setflags(write=False)
    last.setflags(write=False)
    return roots, last


def tree_seed(N):
    return 1700 + N


@functools.lru_cache(maxsize=None)
def tree_case(N, c, prior, with_last):
    roots, last = tree_roots(N)
    return expected_uct_prior(roots, TREE_I, TREE_K, PRIORS[prior], last if with_last else None, c=c, rave_equiv=TREE_EQUIV, fpu=TREE_FPU,
                              komi=TREE_KOMI, base_seed=tree_seed(N))


@functools.lru_cache(maxsize=None)
def rave_case(N, c):
    """The same search without a prior (mc_amaf_expect.expected_uct_rave)."""
    roots, _ = tree_roots(N)
    return ma.expected_uct_rave(roots, TREE_I, TREE_K, c=c, rave_equiv=TREE_EQUIV, fpu=TREE_FPU, komi=TREE_KOMI, base_seed=tree_seed(N))


PAST_N, PAST_I, PAST_EXTRA = 5, 6, 4


@functools.lru_cache(maxsize=None)
def past_capacity_case():
    """A search of PAST_I + PAST_EXTRA iterations on trees with room for PAST_I + 1 nodes."""
    roots, last = tree_roots(PAST_N)
    return expected_uct_prior(roots, PAST_I, TREE_K, DEFAULT, last, c=0.5, rave_equiv=TREE_EQUIV, fpu=TREE_FPU, komi=TREE_KOMI, base_seed=31,
                              iterations=PAST_I + PAST_EXTRA)
