"""Expected results of the PUCT search with several leaves per root per round and virtual loss (gogame.batch_puct(..,
leaves=L) / PuctSearch(.., leaves=L): gg_puct_select_leaves / gg_puct_backup_leaves) - test infrastructure, CPU only.  Builds
on tests/mc_puct_expect.py: LeavesTree is its Tree plus v (the virtual visits), the slot loop with its collisions and the
backup in slot order, written from the text of include/gymgo_amd.h in Python floats (IEEE doubles, the operations of the
specification in its order, math.sqrt)."""
import math

import numpy as np

import mc_expect as mc
import mc_puct_expect as pe
from oracle import c_oracle


def score_vl(s, wc, nc, vc, prior, nx, vx, c):
    """U' of action a at node x: every operation a float64 operation in this order; a NaN counts as -inf."""
    ne = nc + vc
    q = 0.0 if ne == 0 else (s * float(wc) - float(vc)) / float(ne)
    t1 = float(c) * float(prior)
    t2 = math.sqrt(float(nx + vx))
    t3 = t1 * t2
    t4 = t3 / float(1 + ne)
    u = q + t4
    return -math.inf if u != u else u


class LeavesTree(pe.Tree):
    """pe.Tree with room for C + 1 nodes and v per node.  A node created in a round has no board until its backup
    (boards[y] is None in between), as on the device: reading it would be an error here too."""

    def __init__(self, root, C):
        super().__init__(root, C)
        self.v = np.zeros(C + 1, np.int32)
        self.pending = {}      # node created in this round -> its board (what the hand-out plays; stored by the backup)
        self.rounds = []       # per round: [(leaf id, move)] of the L slots, (-1, -1) for an empty one
        self.collisions = 0    # rounds that stopped on a collision
        self.ended_twice = 0   # rounds in which one ended node was taken by two or more slots

    def _walk(self, c):
        """One slot -> (leaf id or -1, move, the board handed out after the move)."""
        x = 0
        while True:
            if self.n[x] == 0 and self.v[x] > 0:            # 1. handed out earlier in this round: a collision
                return -1, -1, None
            acts = self.legal[x]                            # (from here on x has a board)
            if acts.size == 0:                              # 2. the game has ended at x
                return x, -1, self.boards[x]
            if self.n[x] == 0:                              # 3. not evaluated yet
                return x, -1, self.boards[x]
            s = -1.0 if self.boards[x][2, 0, 0] != 0 else 1.0
            best, besta = None, None
            for a in acts:                                  # ascending: strict > keeps the lowest action of equal scores
                k = self.child[x, a]
                nc, wc, vc = (int(self.n[k]), float(self.w[k]), int(self.v[k])) if k >= 0 else (0, 0.0, 0)
                u = score_vl(s, wc, nc, vc, self.prior[x, a], int(self.n[x]), int(self.v[x]), c)
                if best is None or u > best:
                    best, besta = u, int(a)
            k = int(self.child[x, besta])
            if k >= 0:
                x = k
                continue
            if len(self.boards) > self.I:                   # no room (driven past C leaves): x is evaluated as it is
                return x, -1, self.boards[x]
            y = len(self.boards)
            kid = c_oracle.next_state(self.boards[x], besta)
            self.boards.append(None)
            self.legal.append(None)
            self.pending[y] = kid
            self.parent[y], self.action[y], self.child[x, besta] = x, besta, y
            return y, besta, kid

    def select_round(self, c, L):
        """-> [(leaf id, move, board)] of the L slots; empty slots are (-1, -1, a copy of the root)."""
        out, open_ = [], True
        for _ in range(L):
            y, mv, board = self._walk(c) if open_ else (-1, -1, None)
            if y < 0:
                self.collisions += open_
                open_ = False
                out.append((-1, -1, self.boards[0]))
                continue
            z = y
            while z >= 0:
                self.v[z] += 1
                z = self.parent[z]
            out.append((y, mv, board))
        ids = [y for y, _, _ in out if y >= 0 and y not in self.pending and self.legal[y].size == 0]
        self.ended_twice += len(ids) != len(set(ids))
        self.rounds.append([(y, mv) for y, mv, _ in out])
        return out

    def backup_slot(self, y, priors, value, komi):
        if y in self.pending:                               # the board is stored when move >= 0
            self.boards[y] = self.pending.pop(y)
            self.legal[y] = mc.legal_actions(self.boards[y])
        z = y
        while z >= 0:                                       # v -= 1 on the chain, never below 0
            self.v[z] = max(int(self.v[z]) - 1, 0)
            z = self.parent[z]
        self.backup(y, priors, value, komi)                 # priors at n_y = 0, the value, n += 1 and w += v_black


def expected_puct_leaves(roots, T, L, evaluator_np, c=1.25, komi=0.0, on_round=None):
    """-> dict of the outputs of batch_puct(roots, T, evaluator, c, komi, tree=True, leaves=L) (NumPy; pe.ROOT_KEYS, 'tree':
    dict of pe.TREE_KEYS arrays [R, T * L + 1], 'trees': the LeavesTree objects, 'live': per round bool [R, L]).
    evaluator_np(states uint8 [R * L, 6, N, N], legal bool [R * L, A]) -> (priors float32 [R * L, A], values float32 [R * L]).
    on_round(t, trees), if given, is called after every backup."""
    roots = np.ascontiguousarray(roots, np.uint8)
    R, _, N, _ = roots.shape
    A, C = N * N + 1, T * L
    trees = [LeavesTree(roots[r], C) for r in range(R)]
    live = []
    for t in range(T):
        picked = [tr.select_round(c, L) for tr in trees]
        live.append(np.array([[y >= 0 for y, _, _ in row] for row in picked], bool).reshape(R, L))
        if R:
            states = np.stack([b for row in picked for _, _, b in row])
            priors, values = evaluator_np(states, mc.legal_mask(states))
            priors, values = np.asarray(priors, np.float32), np.asarray(values, np.float32)
            assert priors.shape == (R * L, A) and values.shape == (R * L,)
        for r, tr in enumerate(trees):
            for j, (y, _, _) in enumerate(picked[r]):
                if y >= 0:
                    tr.backup_slot(y, priors[r * L + j], values[r * L + j], komi)
        if on_round is not None:
            on_round(t, trees)
    out = {'legal': mc.legal_mask(roots) if R else np.zeros((0, A), bool),
           'visits': np.zeros((R, A), np.int32), 'value_sum': np.zeros((R, A), np.float64),
           'priors': np.zeros((R, A), np.float32)}
    for r, tr in enumerate(trees):
        has = tr.child[0] >= 0
        out['visits'][r, has] = tr.n[tr.child[0, has]]
        out['value_sum'][r, has] = tr.w[tr.child[0, has]]
        out['priors'][r] = tr.prior[0]
    out['root_visits'] = np.array([tr.n[0] for tr in trees], np.int32)
    out['root_value_sum'] = np.array([tr.w[0] for tr in trees], np.float64)
    out['nodes'] = np.array([len(tr.boards) for tr in trees], np.int32)
    stack = lambda f, dt: np.stack([f(tr) for tr in trees]).astype(dt) if R else np.zeros((0, C + 1), dt)
    out['tree'] = {'parent': stack(lambda tr: tr.parent, np.int32), 'action': stack(lambda tr: tr.action, np.int32),
                   'visits': stack(lambda tr: tr.n, np.int32), 'value_sum': stack(lambda tr: tr.w, np.float64)}
    out['trees'] = trees
    out['live'] = live
    return out
