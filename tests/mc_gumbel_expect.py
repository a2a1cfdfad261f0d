"""Expected results of the Gumbel root rule of the PUCT search (gogame.PuctSearch(gumbel=), gumbel_root, puct_play(gumbel=),
puct_selfplay(gumbel=): gg_gumbel_sequence / gg_gumbel_begin / gg_gumbel_select_leaves / gg_gumbel_root) - test infrastructure,
CPU only.  Builds on tests/mc_puct_leaves_expect.py and tests/mc_puct_advance_expect.py: GumbelTree is LeavesTree plus the
per-search state (base, seen, done, the schedule), the root rule and the read-out, written from the text of
include/gymgo_amd_gumbel.h in Python integers and Python floats (IEEE doubles, the operations of the specification in its
order); Search is the host side of gogame.PuctSearch(gumbel=) - when base is refreshed, when the search of a move begins -
and expected_play / expected_selfplay are the move loops of gogame.puct_play / puct_selfplay.

base = g + log(prior) is made by torch on the device and is not bit-defined, so the expectation takes it from outside:
`base_of(search)` is asked whenever gogame refreshes its tensor (before the selects of the first two rounds after a begin or
an advance).  The host tests compute it in NumPy (numpy_base); the device tests hand over what the device made."""
import math

import numpy as np

import mc_expect as mc
import mc_puct_expect as pe
import mc_puct_leaves_expect as pl
import mc_puct_advance_expect as pa
from oracle import c_oracle


def seq(m, n):
    """The schedule of sequential halving, in Python integers, as include/gymgo_amd_gumbel.h states it."""
    assert m >= 1 and n >= 1
    if m == 1:
        return list(range(n))
    lg = 0
    while (1 << lg) < m:
        lg += 1
    k, v, out = m, [0] * m, []
    while len(out) < n:
        e = max(1, n // (lg * k))
        for _ in range(e):
            out.extend(v[:k])
            for i in range(k):
                v[i] += 1
        k = max(2, k // 2)
    return out[:n]


WORKED = {(4, 8): [0, 0, 0, 0, 1, 1, 2, 2], (16, 32): [0] * 16 + [1] * 8 + [2] * 4 + [3] * 4, (3, 7): [0, 0, 0, 1, 1, 2, 2],
          (2, 4): [0, 0, 1, 1], (16, 16): [0] * 16}


class GumbelTree(pl.LeavesTree):
    """pl.LeavesTree with the Gumbel root rule at node 0.  `events` counts what the walks met: 'fallback' (E was empty or the
    schedule was over), 'past' (t >= S), 'tie' (two actions of E with the largest G), 'neg_inf' (an action of E with
    G = -inf), 'collision' (rounds that stopped on one: LeavesTree.collisions)."""

    def __init__(self, root, C, schedule, c_visit, c_scale):
        super().__init__(root, C)
        A = self.prior.shape[1]
        self.schedule, self.c_visit, self.c_scale = list(schedule), float(c_visit), float(c_scale)
        self.base = np.zeros(A, np.float32)
        self.seen = np.zeros(A, np.int64)
        self.done = 0
        self.events = {'fallback': 0, 'past': 0, 'tie': 0, 'neg_inf': 0}

    def begin(self):
        """gg_gumbel_begin: seen = n of node 0's children (every action, legal or not), done = 0."""
        assert not self.pending and not self.v.any()
        self.seen[:] = 0
        for a in range(self.prior.shape[1]):
            k = int(self.child[0, a])
            if k >= 0:
                self.seen[a] = int(self.n[k])
        self.done = 0

    def root_terms(self, with_v):
        """-> (acts, k_a, n_c, qh_a, maxn, q0) over the legal actions of node 0, ascending."""
        acts = [int(a) for a in self.legal[0]]
        s = -1.0 if self.boards[0][2, 0, 0] != 0 else 1.0
        n0 = int(self.n[0])
        q0 = s * float(self.w[0]) / float(n0) if n0 > 0 else 0.0
        ka, ncs, qh = [], [], []
        for a in acts:
            k = int(self.child[0, a])
            nc, wc, vc = (int(self.n[k]), float(self.w[k]), int(self.v[k])) if k >= 0 else (0, 0.0, 0)
            if not with_v:
                assert vc == 0
            ka.append(max(0, nc + vc - int(self.seen[a])))
            ncs.append(nc)
            qh.append(s * wc / float(nc) if nc > 0 else q0)
        return acts, ka, ncs, qh, max(ncs), q0

    def G(self, a, maxn, qh):
        m1 = self.c_visit + float(maxn)
        m2 = m1 * self.c_scale
        sigma = m2 * qh
        g = float(np.float32(self.base[a])) + sigma
        return -math.inf if g != g else g

    def choose(self, need, with_v, count=True):
        """The root rule: need = None is "none".  -> a*."""
        acts, ka, ncs, qh, maxn, _ = self.root_terms(with_v)
        E = [i for i in range(len(acts)) if need is not None and ka[i] == need]
        if not E:
            kmax = max(ka)
            E = [i for i in range(len(acts)) if ka[i] == kmax]
            if count:
                self.events['fallback'] += 1
        best, besta = None, None
        scores = []
        for i in E:                                       # ascending: strict > keeps the lowest action of equal scores
            g = self.G(acts[i], maxn, qh[i])
            scores.append(g)
            if best is None or g > best:
                best, besta = g, acts[i]
        if count:
            self.events['tie'] += scores.count(best) > 1
            self.events['neg_inf'] += -math.inf in scores
        return besta

    def _walk(self, c):
        """One slot: pl.LeavesTree._walk with the root rule in place of step d at node 0."""
        x, ruled = 0, False
        while True:
            if self.n[x] == 0 and self.v[x] > 0:            # a. a collision: done stays
                return -1, -1, None
            acts = self.legal[x]
            if acts.size == 0 or self.n[x] == 0:            # b., c.
                self.done += ruled
                return x, -1, self.boards[x]
            if x == 0:
                t = self.done
                self.events['past'] += t >= len(self.schedule)
                besta = self.choose(self.schedule[t] if t < len(self.schedule) else None, True)
                ruled = True
            else:
                s = -1.0 if self.boards[x][2, 0, 0] != 0 else 1.0
                best, besta = None, None
                for a in acts:
                    k = self.child[x, a]
                    nc, wc, vc = (int(self.n[k]), float(self.w[k]), int(self.v[k])) if k >= 0 else (0, 0.0, 0)
                    u = pl.score_vl(s, wc, nc, vc, self.prior[x, a], int(self.n[x]), int(self.v[x]), c)
                    if best is None or u > best:
                        best, besta = u, int(a)
            k = int(self.child[x, besta])
            if k >= 0:
                x = k
                continue
            self.done += ruled
            if len(self.boards) > self.I:                   # no room
                return x, -1, self.boards[x]
            y = len(self.boards)
            kid = c_oracle.next_state(self.boards[x], besta)
            self.boards.append(None)
            self.legal.append(None)
            self.pending[y] = kid
            self.parent[y], self.action[y], self.child[x, besta] = x, besta, y
            return y, besta, kid

    def readout(self):
        """gg_gumbel_root on one root -> (action, q float32 [A], visits int32 [A], value float32)."""
        assert not self.pending and not self.v.any()
        A = self.prior.shape[1]
        q, visits = np.zeros(A, np.float32), np.zeros(A, np.int32)
        if self.legal[0].size == 0:
            return -1, q, visits, np.float32(0)
        acts, ka, ncs, qh, maxn, q0 = self.root_terms(False)
        for i, a in enumerate(acts):
            q[a], visits[a] = np.float32(qh[i]), ncs[i]
        return self.choose(None, False, count=False), q, visits, np.float32(q0)


def improved_policy(prior, q, visits, legal, c_visit, c_scale):
    """The improved policy of one root in NumPy float64 from the read-out's rows -> float32 [A]: softmax over the legal actions
    of log(prior) + (c_visit + maxn) * c_scale * q; where the largest term is infinite its actions share the mass; +0 on
    illegal actions, a zero row without a legal action."""
    legal = np.asarray(legal, bool)
    out = np.zeros(legal.shape, np.float32)
    if not legal.any():
        return out
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        scale = (float(c_visit) + float(np.asarray(visits).max())) * float(c_scale)
        x = np.log(np.asarray(prior, np.float32).astype(np.float64)) + scale * np.asarray(q, np.float32).astype(np.float64)
        x = np.where(legal & (x == x), x, -np.inf)
        top = x.max()
        e = np.where(legal, np.where(x == top, 1.0, np.exp(x - top)), 0.0)
        out[legal] = (e / e.sum())[legal].astype(np.float32)
    return out


def ulps(a, b):
    """The distance of two float32 arrays in units in the last place (finite values of one sign pattern: probabilities)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def numpy_base(search):
    """base = g + log(prior of node 0) in float32 by NumPy: what gogame makes with torch, up to the logarithm's last bit."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.stack([(search.g[r] + np.log(t.prior[0])).astype(np.float32) for r, t in enumerate(search.trees)])


class Search:
    """The host side of gogame.PuctSearch(gumbel=Gumbel(m, n, c_visit, c_scale), leaves=L) on GumbelTrees."""

    def __init__(self, roots, T, L, m, n=None, c=1.25, komi=0.0, c_visit=50.0, c_scale=0.5, capacity=None, base_of=numpy_base):
        roots = np.ascontiguousarray(roots, np.uint8)
        self.R, self.A = roots.shape[0], roots.shape[-1] ** 2 + 1
        self.T, self.L, self.c, self.komi, self.base_of = T, L or 1, c, komi, base_of
        self.n = max(1, (T - 1) * self.L) if n is None else n
        self.schedule = seq(m, self.n)
        self.c_visit, self.c_scale = c_visit, c_scale
        NN = T * self.L + 1 if capacity is None else capacity
        self.trees = [GumbelTree(roots[r], NN - 1, self.schedule, c_visit, c_scale) for r in range(self.R)]
        self.g = np.zeros((self.R, self.A), np.float32)
        self.rounds = []          # per round since the last begin: (leaf ids [R, L], moves [R, L])
        self.begin()

    def begin(self):
        for t in self.trees:
            t.begin()
        self.since = 0

    def set_g(self, g):
        assert self.since == 0
        self.g = np.asarray(g, np.float32).reshape(self.R, self.A).copy()

    def refresh(self):
        base = np.asarray(self.base_of(self), np.float32)
        for r, t in enumerate(self.trees):
            t.base = base[r].copy()

    def round(self, evaluator_np):
        if self.since < 2:
            self.refresh()
        self.since += 1
        picked = [t.select_round(self.c, self.L) for t in self.trees]
        self.rounds.append((np.array([[y for y, _, _ in row] for row in picked], np.int32).reshape(self.R, self.L),
                            np.array([[mv for _, mv, _ in row] for row in picked], np.int32).reshape(self.R, self.L)))
        if self.R:
            states = np.stack([b for row in picked for _, _, b in row])
            priors, values = evaluator_np(states, mc.legal_mask(states))
            priors, values = np.asarray(priors, np.float32), np.asarray(values, np.float32)
        for r, t in enumerate(self.trees):
            for j, (y, _, _) in enumerate(picked[r]):
                if y >= 0:
                    t.backup_slot(y, priors[r * self.L + j], values[r * self.L + j], self.komi)

    def readout(self):
        """-> (actions int32 [R], q float32 [R, A], visits int32 [R, A], value float32 [R], pi float32 [R, A])."""
        if self.since < 2:
            self.refresh()
        rows = [t.readout() for t in self.trees]
        acts = np.array([a for a, _, _, _ in rows], np.int32).reshape(self.R)
        q = np.stack([x for _, x, _, _ in rows]) if self.R else np.zeros((0, self.A), np.float32)
        vis = np.stack([x for _, _, x, _ in rows]) if self.R else np.zeros((0, self.A), np.int32)
        val = np.array([x for _, _, _, x in rows], np.float32).reshape(self.R)
        pi = np.zeros((self.R, self.A), np.float32)
        for r, t in enumerate(self.trees):
            legal = np.zeros(self.A, bool)
            legal[t.legal[0]] = True
            pi[r] = improved_policy(t.prior[0], q[r], vis[r], legal, self.c_visit, self.c_scale)
        return acts, q, vis, val, pi

    def advance(self, acts):
        kept = [pa.advance(t, int(a), pa.next_root(t, int(a))) for t, a in zip(self.trees, acts)]
        self.begin()
        return kept

    def state(self):
        """What the device tests compare exactly: the tree, done and seen."""
        NN = self.trees[0].n.shape[0] if self.R else 0
        stack = lambda f, dt: np.stack([f(t) for t in self.trees]).astype(dt) if self.R else np.zeros((0, NN), dt)
        return {'parent': stack(lambda t: t.parent, np.int32), 'action': stack(lambda t: t.action, np.int32),
                'n': stack(lambda t: t.n, np.int32), 'w': stack(lambda t: t.w, np.float64), 'v': stack(lambda t: t.v, np.int32),
                'child': stack(lambda t: t.child, np.int32), 'prior': stack(lambda t: t.prior, np.float32),
                'nodes': np.array([len(t.boards) for t in self.trees], np.int32),
                'done': np.array([t.done for t in self.trees], np.int32),
                'seen': stack(lambda t: t.seen, np.int32)}

    def events(self):
        out = {k: sum(t.events[k] for t in self.trees) for k in ('fallback', 'past', 'tie', 'neg_inf')}
        out['collision'] = sum(t.collisions for t in self.trees)
        return out


def expected_gumbel(roots, T, L, evaluator_np, m, **kw):
    """T rounds from fresh roots -> the Search (its trees, rounds, readout())."""
    s = Search(roots, T, L, m, **kw)
    for _ in range(T):
        s.round(evaluator_np)
    return s


def expected_play(roots, moves, T, L, evaluator_np, m, reuse=True, g_of=None, **kw):
    """gogame.puct_play(gumbel=) restated -> (actions int64 [R, moves], final states, the last Search).  g_of(mv, legal) or None."""
    roots = np.ascontiguousarray(roots, np.uint8)
    s = Search(roots, T, L, m, **kw)
    played = np.zeros((s.R, moves), np.int64)
    for mv in range(moves):
        if g_of is not None:
            s.set_g(g_of(mv, np.stack([_legal_row(t, s.A) for t in s.trees])))
        for _ in range(T):
            s.round(evaluator_np)
        acts = s.readout()[0]
        played[:, mv] = acts
        if reuse:
            s.advance(acts)
        else:
            nxt = np.stack([pa.next_root(t, int(a)) for t, a in zip(s.trees, acts)])
            s = Search(nxt, T, L, m, **kw)
    return played, np.stack([t.boards[0] for t in s.trees]), s


def _legal_row(tree, A):
    row = np.zeros(A, bool)
    row[tree.legal[0]] = True
    return row


def expected_selfplay(roots, moves, T, L, evaluator_np, m, g_of, **kw):
    """gogame.puct_selfplay(gumbel=, gumbel_noise=g_of) restated -> dict of actions int64 [R, moves], pi float32 [R, moves, A],
    value float32 [R, moves], lengths int32 [R], final_states."""
    roots = np.ascontiguousarray(roots, np.uint8)
    s = Search(roots, T, L, m, **kw)
    out = {'actions': np.full((s.R, moves), -1, np.int64), 'pi': np.zeros((s.R, moves, s.A), np.float32),
           'value': np.zeros((s.R, moves), np.float32), 'lengths': np.zeros(s.R, np.int32)}
    for mv in range(moves):
        if g_of is not None:
            s.set_g(g_of(mv, np.stack([_legal_row(t, s.A) for t in s.trees])))
        for _ in range(T):
            s.round(evaluator_np)
        acts, _, _, val, pi = s.readout()
        out['actions'][:, mv], out['pi'][:, mv], out['value'][:, mv] = acts, pi, val
        out['lengths'] += acts >= 0
        s.advance(acts)
    out['final_states'] = np.stack([t.boards[0] for t in s.trees])
    out['search'] = s
    return out


# ---------------------------------------------------------------- the cases of tests/test_gpu_gumbel.py
EVALUATORS = {'hash': (pe.hash_evaluator_np, pe.hash_evaluator_t), 'hostile': (pe.hostile_evaluator_np, pe.hostile_evaluator_t),
              'pass': (pe.pass_evaluator_np, pe.pass_evaluator_t)}
SIZE_NAMES = ('mid0', 'late0', 'late1', 'passed', 'ended')      # five roots at every size: mid-game, few legal actions, an ended game
SIZE_ROUNDS, SIZE_M = 6, 4
SLOT_SIZES, SLOT_LEAVES, SLOT_ROUNDS = (5, 9, 19), (1, 3, 8), 9
SLOT_NAMES = ('mid0', 'late0', 'ended')


def slot_considered(N):
    return (1, 2, 4, 16, N * N + 1 + 5)


def size_case(N, L):
    """-> (roots, evaluator name): the evaluators take turns over the sizes."""
    import mc_cases as cs
    return cs.stack(N, SIZE_NAMES), ('hash', 'hostile', 'pass')[(N + L) % 3]


def slot_case(N, L, m):
    import mc_cases as cs
    return cs.stack(N, SLOT_NAMES), ('hash', 'hostile')[(L + m) % 2]


def dyadic_g(R, A, mv=0, salt=0):
    """float32 [R, A]: draws that are exact in float32 (multiples of 1/64 in [-2, 6)), a function of (row, action, move)."""
    r, a = np.arange(R, dtype=np.int64)[:, None], np.arange(A, dtype=np.int64)[None, :]
    k = ((r * 7919 + a * 104729 + (mv + 1) * 1299709 + salt * 15485863) * 2654435761 >> 11) % 512
    return (k.astype(np.float32) - np.float32(128)) / np.float32(64)
