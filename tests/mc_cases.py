"""Roots for the Monte Carlo and tree-search stack at every board size from 2 to 19 (tests/test_gpu_mc_sizes.py; the premises the
device tests rely on are asserted on the CPU by tests/test_mc_cases_host.py) - test infrastructure, CPU only, built with the C
restatement under oracle/ and the helpers of tests/mc_expect.py and tests/mc_policy_expect.py.  Everything is a function of
(N, seed) alone."""
import functools

import numpy as np

import mc_expect as mc
import mc_policy_expect as mp
from oracle import c_oracle

SIZES = tuple(range(2, 20))
LATE_GAMES = 64          # oracle games stepped side by side until three of them are late
LATE_POINTS = 6          # a late root has 1 .. LATE_POINTS legal points (and the pass)
UCT_I, UCT_K = 24, 2     # the UCT search of the device test: deep enough below every late root (test_mc_cases_host.py)


def late_roots(N, seed=0, count=3):
    """`count` live positions with 1 .. LATE_POINTS legal points: LATE_GAMES games of random play by the restatement from the
    empty board, one ply at a time; from ply N^2 / 2 on, the first live boards (lowest ply, then lowest game; one per game)
    with so few legal points.  With so few actions a search of a few dozen iterations gives every action of a node a child
    and walks on below it."""
    states = np.zeros((LATE_GAMES, 6, N, N), np.uint8)
    rng = c_oracle.rng_seed(1000 + 37 * N + seed, LATE_GAMES)
    out, taken = [], set()
    for ply in range(8 * N * N + 64):
        if ply >= N * N // 2:
            live = states[:, 5, 0, 0] == 0
            points = (states[:, 3] == 0).sum(axis=(1, 2))
            for g in np.flatnonzero(live & (points >= 1) & (points <= LATE_POINTS)):
                if int(g) not in taken:
                    taken.add(int(g))
                    out.append(states[g].copy())
                    if len(out) == count:
                        return np.stack(out)
        states, rng, _ = c_oracle.batch_rollout(states, rng, 1, auto_reset=False)
    raise AssertionError('no %d late roots at N = %d, seed %d' % (count, N, seed))


def small_crafted_roots(N):
    """The hand-made roots of the two sizes too small for mc.crafted_roots (2 and 3: no room for its ko): [the empty board,
    black plays and white passes (the pass child is terminal), two passes (a finished game)].  These sizes have NO ko root."""
    empty = np.zeros((6, N, N), np.uint8)
    passed = c_oracle.next_state(c_oracle.next_state(empty, (N // 2) * N + N // 2), N * N)
    end = c_oracle.next_state(c_oracle.next_state(empty, N * N), N * N)
    assert passed[4].all() and not passed[5].any() and end[5].all()
    return np.stack([empty, passed, end])


@functools.lru_cache(maxsize=None)
def _size_roots(N):
    rand = mc.make_roots(N, 4, 70 + N, max_ply=N * N // 2, step=max(2, N * N // 8))
    late = late_roots(N)
    forced = mp.forced_pass_roots(N)
    named = [('mid0', rand[1]), ('mid1', rand[2]), ('late0', late[0]), ('late1', late[1]), ('late2', late[2])]
    if N >= 4:
        named += list(zip(('empty', 'passed', 'ko', 'ended'), mc.crafted_roots(N)))
    else:
        named += list(zip(('empty', 'passed', 'ended'), small_crafted_roots(N)))
    named += [('forced_black', forced[0]), ('forced_white', forced[1]), ('played_out', rand[3])]
    for _, r in named:
        r.setflags(write=False)
    return tuple(named)


def size_roots(N):
    """The named roots of size N, in a fixed order -> dict name -> uint8 [6, N, N] (read-only; at most 12):
    mid0, mid1      two positions of random play (mc.make_roots)
    late0 .. late2  late_roots(N)
    empty, passed, ko, ended   mc.crafted_roots(N) for N >= 4; at 2 and 3 small_crafted_roots(N), which has no ko
    forced_black, forced_white mp.forced_pass_roots(N): the mover has no candidate, both boards carry eyes
    played_out      a game of random play played to its end (the last root of mc.make_roots)"""
    return dict(_size_roots(N))


def stack(N, names=None):
    """uint8 [R, 6, N, N]: the roots `names` (default: all of them, in size_roots' order)."""
    roots = size_roots(N)
    return np.stack([roots[k] for k in (names if names is not None else roots)])


def search_names(N):
    """The roots of the UCT case: the late roots and one mid-game root."""
    return ('late0', 'late1', 'late2', 'mid0')


def move_names(N):
    """The roots of the flat Monte Carlo case: one mid-game root, one late root, one finished game."""
    return ('mid0', 'late0', 'ended')


def full_cap(N, chunk_plies=32):
    """The default max_plies of the playouts: 8 N^2 rounded up to the chunk length (32: a multiple of every chunk used)."""
    return -(-8 * N * N // chunk_plies) * chunk_plies


def deep_nodes(parent):
    """How many nodes of a tree (its parent vector, -1 at the root and at unused nodes) have a parent that is not the root."""
    return int((np.asarray(parent) > 0).sum())


# ---------------------------------------------------------------- the cases of tests/test_gpu_mc_sizes.py
PLAYOUT_K = 4
PLAYOUT_TILES = 5        # the size's roots five times over: 55 / 60 roots x 4 playouts, more jobs than the 200 slots of the device test
SLOTS = (24, 200)
CHUNKS = (8, 32)
ADVANCE_T = 6
TREE_CASES = ((None, 'hash'), (4, 'hostile'))      # (leaves, evaluator) of the advance and the self-play pieces
ALL_KINDS = frozenset(('most', 'least', 'unvisited', 'stay', 'ended'))


def playout_roots(N):
    """The roots of the playout case: every root PLAYOUT_TILES times (each copy has its own jobs, so its own playouts)."""
    return np.tile(stack(N), (PLAYOUT_TILES, 1, 1, 1))


def tiled(N, B):
    """B boards: the size's roots over and over."""
    s = stack(N)
    return s[np.arange(B) % len(s)].copy()


def puct_iterations(N):
    return min(2 * (N * N + 1), 80)


def scored_names(N):
    """The roots whose searches score finished games on the device: the two finished roots, and the boards black fills but
    for two eyes (a pass and a pass below them end the game on a full board)."""
    return ('ended', 'played_out', 'forced_black', 'forced_white')


def advance_kinds(N, L):
    """What test_gpu_puct_advance._mixed_actions yields on the size's roots after ADVANCE_T rounds (asserted by
    tests/test_mc_cases_host.py): all five kinds, except at N = 2 with four leaves a round, where 24 slots give every
    legal action of every root (five at most) a child - no 'unvisited' action, so no fresh tree."""
    return ALL_KINDS - {'unvisited'} if N == 2 and L is not None else ALL_KINDS


def noise_kinds(N, L):
    """What the move of test_gpu_puct_selfplay.noise_and_policy_on_searched_trees leaves among the size's roots: ended, kept
    and fresh trees (the same exception as advance_kinds)."""
    return frozenset(('ended', 'kept')) if N == 2 and L is not None else frozenset(('ended', 'kept', 'fresh'))
