"""Expected results of the UCT search with several leaves per root and round (gogame.batch_uct(leaves=L);
include/gymgo_amd_uct_leaves.h holds the rule) - test infrastructure, CPU only, built on tests/mc_expect.py (Tree, the
playouts), tests/mc_amaf_expect.py (RaveTree, the AMAF playouts) and tests/mc_prior_expect.py (PriorTree).

Leaves is a mixin over the three tree classes: v, the slot loop with its collisions, nodes that count as board-less until their
backup, and the backup in slot order.  The scores are mc_expect.score and mc_amaf_expect.rave_u, the expressions of the one-leaf
restatements, with n_c + K v_c for n and log_table[n_x / K + v_x].  The cases the device tests run are functions of their
arguments alone and cached, so tests/test_uct_leaves_host.py (their premises) and tests/test_gpu_uct_leaves.py (the comparison)
share one computation."""
import functools
import math

import numpy as np

import mc_amaf_expect as ma
import mc_cases as cs
import mc_expect as mc
import mc_prior_expect as mq
from oracle import c_oracle


class Leaves:
    """Over mc.Tree / ma.RaveTree / mq.PriorTree, built with I = C = rounds * L."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.C = len(self.parent) - 1
        self.rave = hasattr(self, 'node_amaf')
        self.v = np.zeros(self.C + 1, np.int64)
        self.boardless = set()          # the nodes made in the current round: no board until their backup
        # for the premises: what the slots of every round did
        self.log = []                   # per round: list of (kind, depth, leaf id), kind in expand / ended / noroom / empty
        self.collisions = 0             # slots that met a collision themselves
        self.vl_changed = 0             # choices that differ from what v = 0 everywhere would have chosen
        self.path_counts = None         # v between the select and the backup of the last round

    def chain(self, y):
        while y >= 0:
            yield int(y)
            y = self.parent[y]

    def choose(self, x, K, c, Ltab, k, fpu, v):
        """The action node x chooses under the virtual visits v -> action."""
        acts = self.legal[x]
        white = self.boards[x][2, 0, 0] != 0
        t = int(self.stats[x, 0] // K) + int(v[x])
        lx = Ltab[min(max(t, 0), self.C)]
        if not self.rave:
            free = acts[self.child[x, acts] < 0]
            if free.size:
                return int(free[0])
        best, besta = None, None
        for a in acts:                         # ascending: strict > keeps the lowest action of equal scores
            ch = int(self.child[x, a])
            n = s = w = d = 0
            if ch >= 0:
                n0, bw, ww, d = (int(q) for q in self.stats[ch])
                n, w = n0 + K * int(v[ch]), (ww if white else bw)
                s = 2 * w + d
            if self.rave:
                nt, st = (int(q) for q in self.node_amaf[x, a]) if a < self.P else (0, 0)
                u = ma.rave_u(n, s, nt, st, lx, c, k, fpu)
            else:
                u = mc.score(w, d, n, lx, c)
            if best is None or u > best:
                best, besta = u, int(a)
        return besta

    def select_slot(self, K, c, Ltab, k=None, fpu=None):
        """One slot's walk -> (leaf id, the board the playouts start from, move, kind, depth) or None for a collision."""
        x, depth = 0, 0
        zero = np.zeros_like(self.v)
        while True:
            assert (x in self.boardless) == (x > 0 and self.stats[x, 0] == 0)
            if x > 0 and self.stats[x, 0] == 0:            # before any look at x's board
                return None
            if self.legal[x].size == 0:
                return x, self.boards[x], -1, 'ended', depth
            a = self.choose(x, K, c, Ltab, k, fpu, self.v)
            if self.rave and self.v.any() and a != self.choose(x, K, c, Ltab, k, fpu, zero):   # (plain: a child of this round has n = 0)
                self.vl_changed += 1
            ch = int(self.child[x, a])
            if ch < 0:
                y = len(self.boards)
                if y > self.C:                              # no room left: x is evaluated as it is
                    return x, self.boards[x], -1, 'noroom', depth
                kid = c_oracle.next_state(self.boards[x], a)
                self.boards.append(kid)
                self.legal.append(mc.legal_actions(kid))
                self.parent[y], self.action[y], self.child[x, a] = x, a, y
                self.boardless.add(y)
                if hasattr(self, 'weights'):                # a PriorTree: the new node's pairs, the expanded action its previous one
                    if self.first_expanded is None:
                        self.first_expanded = a
                    self.node_amaf[y] += mq.prior_pairs(kid[None], [a], self.weights)[0]
                if self.rave:
                    self.max_depth = max(self.max_depth, depth + 1)
                return y, kid, a, 'expand', depth
            x, depth = ch, depth + 1

    def select_round(self, L, *sel):
        """-> L slots (leaf id, board, move): (-1, the root's board, -1) for the empty ones."""
        assert not self.v.any() and not self.boardless
        slots, events, open_ = [], [], True
        for j in range(L):
            got = self.select_slot(*sel) if open_ else None
            if got is None:
                self.collisions += open_
                open_ = False
                slots.append((-1, self.boards[0], -1))
                events.append(('empty', 0, -1))
                continue
            y, board, move, kind, depth = got
            for z in self.chain(y):
                self.v[z] += 1
            slots.append((y, board, move))
            events.append((kind, depth, y))
        self.log.append(events)
        self.path_counts = self.v.copy()
        return slots

    def backup_round(self, slots, K, e, row0):
        """The slots of a round in ascending order, e: the playouts of every row, row0: this tree's first row."""
        for j, (y, _, _) in enumerate(slots):
            if y < 0:
                continue
            self.boardless.discard(y)
            self.update(y, K, e, row0 + j)
            for z in self.chain(y):
                self.v[z] = max(self.v[z] - 1, 0)
        assert not self.v.any() and not self.boardless


class LeavesTree(Leaves, mc.Tree):
    pass


class LeavesRaveTree(Leaves, ma.RaveTree):
    pass


class LeavesPriorTree(Leaves, mq.PriorTree):
    pass


def run_uct_leaves(trees, roots, rounds, L, K, sel, playouts, max_plies, komi, base_seed, first_root, chunk_plies, after_select=None):
    """mc_expect.run_uct for L slots per root and round: the R L rows (row r L + j = slot j of root r) are evaluated together,
    at first_root L, with the seed of round t; only non-empty rows reach the trees and the totals.  after_select(t, trees): a
    look at the trees between a round's select and its backup.  -> run_uct's dict, plus 'live' (int [rounds, R]: the
    non-empty slots)."""
    R, _, N, _ = roots.shape
    if max_plies is None:
        max_plies = -(-8 * N * N // chunk_plies) * chunk_plies
    unfinished, plies = np.zeros(R, np.int64), np.zeros(R, np.int64)
    live = np.zeros((rounds, R), np.int64)
    for t in range(rounds):
        picked = [tr.select_round(L, *sel) for tr in trees]
        if after_select is not None:
            after_select(t, trees)
        rows = np.stack([s[1] for p in picked for s in p])
        e = playouts(rows, K, max_plies, komi=komi, base_seed=int(mc.po_seed(base_seed, t)), first_root=first_root * L)
        for r, tr in enumerate(trees):
            tr.backup_round(picked[r], K, e, r * L)
            for j, (y, _, _) in enumerate(picked[r]):
                if y >= 0:
                    live[t, r] += 1
                    unfinished[r] += e['unfinished'][r * L + j]
                    plies[r] += e['plies_sum'][r * L + j]
    out = mc.run_uct(trees, roots, 0, K, sel, playouts, max_plies, komi, base_seed, first_root, chunk_plies)   # (the assembly alone)
    out['unfinished'], out['plies_sum'], out['live'] = unfinished, plies, live
    return out


def expected_uct_leaves(roots, T, L, K, c=math.sqrt(2), rave=None, prior=None, max_plies=None, komi=0.0, base_seed=20260927,
                        first_root=0, chunk_plies=32, policy=0, rollout=None, after_select=None, capacity=None):
    """-> dict of the outputs of batch_uct(roots, T, K, leaves=L, tree=True) (NumPy; mc_expect.ROOT_KEYS, 'tree', 'trees', 'live').
    rave: None or (rave_equiv, fpu) - then 'rave_visits', 'rave_score' and 'node_amaf' in 'tree' as well, the playouts under
    `policy` (0 / 1 / 2); without it the playouts use `rollout` (mc_expect.replay's).  prior (with rave): None or (weights,
    last_actions or None).  'child' is in 'tree' in every mode.  capacity: the leaves a tree has room for (default T L; less: a
    search past its capacity, whose slots evaluate the node they stand at once the tree is full)."""
    roots = np.ascontiguousarray(roots, np.uint8)
    C = T * L if capacity is None else capacity
    if rave is None:
        assert prior is None
        trees = [LeavesTree(root, C) for root in roots]
        sel, po = (K, c, mc.log_table(C, K)), functools.partial(mc.expected_playouts, rollout=rollout)
    else:
        if prior is None:
            trees = [LeavesRaveTree(root, C) for root in roots]
        else:
            w, last = prior
            trees = [LeavesPriorTree(roots[r], C, w, None if last is None else int(last[r])) for r in range(len(roots))]
        sel, po = (K, c, mc.log_table(C, K), rave[0], rave[1]), functools.partial(ma.expected_playouts_amaf, policy=policy)
    out = run_uct_leaves(trees, roots, T, L, K, sel, po, max_plies, komi, base_seed, first_root, chunk_plies, after_select)
    if rave is not None:
        out['tree']['node_amaf'] = na = np.stack([t.node_amaf for t in trees]).astype(np.int32)
        out['rave_visits'], out['rave_score'] = na[:, 0, :, 0], na[:, 0, :, 1]
    out['tree']['child'] = np.stack([t.child for t in trees]).astype(np.int32)
    return out


def keys(mode):
    """(root keys, tree keys) of a mode's results."""
    return (mc.ROOT_KEYS, mc.TREE_KEYS) if mode == 'plain' else (ma.RAVE_ROOT_KEYS, ma.RAVE_TREE_KEYS)


# ---------------------------------------------------------------- the cases of the device tests
MODES = ('plain', 'rave', 'prior')
SIZES = tuple(range(2, 20))
LS = (1, 2, 4, 8)
EQUIV, FPU, KOMI = 50.0, 0.5, 0.5
WEIGHTS = mq.LOPSIDED


def mode_args(mode, R, N):
    """-> (rave, prior) of expected_uct_leaves for a mode; the prior's last actions: a point, the pass, none, in turn."""
    if mode == 'plain':
        return None, None
    if mode == 'rave':
        return (EQUIV, FPU), None
    return (EQUIV, FPU), (WEIGHTS, np.array([(N * N // 2, N * N, -1)[r % 3] for r in range(R)], np.int32))


def size_shape(N):
    """(T, K, max_plies, root names) of the size's case: small enough for the CPU restatement to take a few seconds, the
    playouts one chunk of 32 plies (N >= 13) or two."""
    if N >= 13:
        return 4, 1, 32, ('late0', 'mid0')
    if N >= 7:
        return 5, 2, 64, ('late0', 'mid0', 'ended')
    return 6, 2, 64, ('late0', 'late1', 'empty', 'ended')


def size_L(N, mode):
    """The slot counts a size runs in a mode: all of LS, at every size and in every mode."""
    return LS


def size_c(mode):
    """Plain: sqrt 2.  RAVE: 0.4, so that the exploration term of a child handed out in this round, c sqrt(log K / K), stays below
    FPU and a round's later slots expand other actions instead of walking into it (c_case has the other values of c)."""
    return math.sqrt(2) if mode == 'plain' else 0.4


def size_seed(N):
    return 4000 + N


@functools.lru_cache(maxsize=None)
def size_case(N, mode, L, policy=0):
    T, K, cap, names = size_shape(N)
    roots = cs.stack(N, names)
    rave, prior = mode_args(mode, len(roots), N)
    return roots, expected_uct_leaves(roots, T, L, K, c=size_c(mode), rave=rave, prior=prior, max_plies=cap, komi=KOMI, base_seed=size_seed(N),
                                      policy=policy)


def all_size_cases():
    return [(N, mode, L) for N in SIZES for mode in MODES for L in size_L(N, mode)]


ENDED_N, ENDED_T, ENDED_K = 5, 12, 2


def ended_roots():
    """5x5: the root whose pass child ends the game, and a late root."""
    return cs.stack(ENDED_N, ('passed', 'late0'))


@functools.lru_cache(maxsize=None)
def ended_case(mode, L):
    """5x5 with ended nodes inside the tree (the pass below `passed` ends the game): c = 0.3."""
    roots = ended_roots()
    rave, prior = mode_args(mode, len(roots), ENDED_N)
    return roots, expected_uct_leaves(roots, ENDED_T, L, ENDED_K, c=0.3, rave=rave, prior=prior, max_plies=64, komi=KOMI, base_seed=77)


BIG_C = 1e6


@functools.lru_cache(maxsize=None)
def c_case(mode, c, L=8):
    """5x5, c in {0, sqrt 2, 1e6} on two late roots and a mid-game root: the late roots run out of actions without a child in the
    middle of a round, and the slot after that walks into a node of its own round."""
    roots = cs.stack(5, ('late0', 'late1', 'mid0'))
    rave, prior = mode_args(mode, len(roots), 5)
    return roots, expected_uct_leaves(roots, 6, L, 2, c=c, rave=rave, prior=prior, max_plies=64, komi=KOMI, base_seed=91)


@functools.lru_cache(maxsize=None)
def wide_case(mode):
    """L = 64 at 9x9: two rounds on two roots."""
    roots = cs.stack(9, ('mid0', 'late0'))
    rave, prior = mode_args(mode, len(roots), 9)
    return roots, expected_uct_leaves(roots, 2, 64, 2, c=size_c(mode), rave=rave, prior=prior, max_plies=32, komi=KOMI, base_seed=64)


def kinds(tree):
    """Per round the set of (kind, descended or not) of a tree's slots."""
    return [{(k, d > 0) for k, d, _ in ev} for ev in tree.log]


def ended_twice(tree):
    """Rounds in which one ended node was taken by two slots."""
    n = 0
    for ev in tree.log:
        ids = [y for k, _, y in ev if k == 'ended']
        n += len(ids) != len(set(ids))
    return n


PAST_T, PAST_L, PAST_K, PAST_C = 4, 4, 2, 9


@functools.lru_cache(maxsize=None)
def past_capacity_case(mode):
    """5x5: four rounds of four slots on trees with room for 9 leaves."""
    roots = cs.stack(5, ('late0', 'mid0', 'ended'))
    rave, prior = mode_args(mode, len(roots), 5)
    return roots, expected_uct_leaves(roots, PAST_T, PAST_L, PAST_K, c=size_c(mode), rave=rave, prior=prior, max_plies=64, komi=KOMI,
                                      base_seed=13, capacity=PAST_C)
