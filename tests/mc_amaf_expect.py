"""Expected results of the AMAF statistics of the playout queue and of the RAVE search (gogame.batch_rollout_tracked_log,
batch_playouts(amaf=True), batch_uct(rave_equiv=...); include/gymgo_amd_amaf.h) - test infrastructure, CPU only, beside
tests/mc_expect.py.  The move sequence of every playout comes from the restatements ONE PLY PER CALL (the C restatement under
oracle/ for the uniform policy, mc_policy_expect / mc_tactics_expect for the other two), the first-play maps and their
reduction are NumPy, the search is restated in Python (RaveTree: the value and U in Python floats - IEEE doubles, the same
operations in the same order, math.sqrt).  The cases the device tests run are functions of their arguments alone and cached,
so tests/test_amaf_host.py (their premises) and tests/test_gpu_amaf.py (the comparison) share one computation."""
import functools
import math

import numpy as np

import mc_cases as cs
import mc_expect as mc
import mc_policy_expect as mp
import mc_tactics_expect as mt
from oracle import c_oracle

POLICIES = ('uniform', 'no_eye_fill', 'tactical')
SIZES = tuple(range(2, 20))
UNWRITTEN = -1          # int16 view of the 0xFFFF the log holds beforehand


# ---------------------------------------------------------------- move sequences
def one_ply(states, rng, policy):
    """One ply of every live game under playout policy 0 / 1 / 2, no auto-reset -> (states, rng, actions int32 [B], -1 where the
    game had ended)."""
    if policy == 0:
        return c_oracle.batch_rollout(states, rng, 1, auto_reset=False)
    st, rng, last, _ = (mp.policy_rollout if policy == 1 else mt.tactical_rollout)(states, rng, 1, auto_reset=False)
    return st, rng, last


def play_sequences(states, rng, plies, policy=0):
    """Up to `plies` plies of every game, one ply per call -> (final states, generators, actions int32 [B, plies] with -1 for the
    plies a game did not play, plies played int64 [B])."""
    cur = np.array(states, np.uint8, copy=True)
    rng = np.array(rng, np.uint64, copy=True)
    B = cur.shape[0]
    acts = np.full((B, int(plies)), -1, np.int32)
    for t in range(int(plies)):
        if (cur[:, 5, 0, 0] != 0).all():
            break
        cur, rng, last = one_ply(cur, rng, policy)
        acts[:, t] = last
    played = (acts >= 0).sum(axis=1).astype(np.int64)
    assert ((acts >= 0) == (np.arange(int(plies))[None, :] < played[:, None])).all()     # live plies are a prefix
    return cur, rng, acts, played


# ---------------------------------------------------------------- first-play maps
def first_play_maps(acts, start_white, N):
    """bool [B, 2, N*N]: the points black / white played first in each move sequence (acts int32 [B, T], -1: no ply; N*N: the
    pass; ply t is played by the starting colour flipped t times)."""
    acts = np.asarray(acts)
    B, T = acts.shape
    P = N * N
    taken = np.zeros((B, P), bool)
    out = np.zeros((B, 2, P), bool)
    idx = np.arange(B)
    for t in range(T):
        a = acts[:, t]
        m = (a >= 0) & (a < P)
        if not m.any():
            continue
        rows, pts = idx[m], a[m]
        fresh = ~taken[rows, pts]
        rows, pts = rows[fresh], pts[fresh]
        col = (np.asarray(start_white, bool)[rows] ^ bool(t & 1)).astype(int)
        out[rows, col, pts] = True
        taken[rows, pts] = True
    return out


def sequence_facts(acts, start_white, N):
    """Per sequence: (a point is played again by the OTHER colour than the one that played it first, a pass stands before the
    last two plies)."""
    acts = np.asarray(acts)
    P = N * N
    replay = np.zeros(len(acts), bool)
    early_pass = np.zeros(len(acts), bool)
    for b, row in enumerate(acts):
        row = row[row >= 0]
        owner = {}
        for t, a in enumerate(row):
            c = bool(start_white[b]) ^ bool(t & 1)
            if a < P:
                if a in owner and owner[a] != c:
                    replay[b] = True
                owner.setdefault(int(a), c)
        early_pass[b] = bool((row[:-2] == P).any()) if len(row) > 2 else False
    return replay, early_pass


def expected_playouts_amaf(roots, K, max_plies, komi=0.0, base_seed=20260927, first_root=0, with_ownership=False, policy=0):
    """-> dict of the per-root outputs of batch_playouts(amaf=True, policy=...) (NumPy): mc_expect.KEYS, 'ownership', 'amaf'
    (int32 [R, 2, 3, N, N]); and, for the premises, 'sequences' (int32 [R K, max_plies]), 'maps' (bool [R K, 2, N*N])."""
    roots = np.ascontiguousarray(roots, np.uint8)
    R, _, N, _ = roots.shape
    jobs = first_root * K + np.arange(R * K)
    rng0 = mc.po_seed(base_seed, jobs)
    starts = np.repeat(roots, K, axis=0)
    fin, rng1, acts, played = play_sequences(starts, rng0, max_plies, policy)
    assert np.array_equal(mc.plies_from_rng(rng0, rng1), played)
    b, w = c_oracle.batch_areas_mt(fin)
    d = np.asarray(b, np.int64) - np.asarray(w, np.int64)
    x = d - komi
    ended = fin[:, 5, 0, 0] != 0
    per = lambda v: np.asarray(v, np.int64).reshape(R, K).sum(axis=1)
    out = {'black_wins': per(x > 0).astype(np.int32), 'white_wins': per(x < 0).astype(np.int32), 'draws': per(x == 0).astype(np.int32),
           'unfinished': per(~ended).astype(np.int32), 'margin_sum': per(d), 'plies_sum': per(played), 'ownership': None}
    if with_ownership:
        out['ownership'] = mc.ownership(fin).astype(np.int32).reshape(R, K, 2, N, N).sum(axis=1).astype(np.int32)
    start_white = starts[:, 2, 0, 0] != 0
    maps = first_play_maps(acts, start_white, N)
    amaf = np.zeros((R, 2, 3, N * N), np.int64)
    for k, sel in enumerate((np.ones(R * K, bool), x > 0, x < 0)):
        amaf[:, :, k] = (maps & sel[:, None, None]).reshape(R, K, 2, N * N).sum(axis=1)
    out['amaf'] = amaf.reshape(R, 2, 3, N, N).astype(np.int32)
    out['sequences'], out['maps'], out['start_white'] = acts, maps, start_white
    return out


# ---------------------------------------------------------------- RAVE
def rave_value(n, s, nt, st, k, fpu):
    """The value of an action: n, s = 2 w + d of its child (0 without one), nt, st of the node's AMAF pair; each operation a
    float64 operation in the order written."""
    if n > 0 and nt > 0:
        q = float(s) / (2.0 * float(n))
        qt = float(st) / (2.0 * float(nt))
        beta = float(nt) / (float(n) + float(nt) + (float(n) * float(nt)) / float(k))
        return (1.0 - beta) * q + beta * qt
    if n > 0:
        return float(s) / (2.0 * float(n))
    if nt > 0:
        return float(st) / (2.0 * float(nt))
    return float(fpu)


def rave_u(n, s, nt, st, log_nx, c, k, fpu):
    v = rave_value(n, s, nt, st, k, fpu)
    return v + float(c) * math.sqrt(float(log_nx) / float(n)) if n > 0 else v


class RaveTree(mc.Tree):
    def __init__(self, root, I):
        super().__init__(root, I)
        N = root.shape[-1]
        self.I, self.P = I, N * N
        self.node_amaf = np.zeros((I + 1, N * N, 2), np.int64)
        self.max_depth = 0
        self.replayed = 0      # the iterations in which a point of a tree move on the path was played again in a playout below it

    def select(self, K, c, L, k, fpu):
        """-> (leaf id, leaf board, new node or not)."""
        x, depth = 0, 0
        while True:
            acts = self.legal[x]
            if acts.size == 0:
                return x, self.boards[x], False
            white = self.boards[x][2, 0, 0] != 0
            lx = L[min(int(self.stats[x, 0] // K), self.I)]
            best, besta = None, None
            for a in acts:
                ch = self.child[x, a]
                n = s = 0
                if ch >= 0:
                    n, bw, ww, d = (int(v) for v in self.stats[ch])
                    s = 2 * (ww if white else bw) + d
                nt, st = (int(v) for v in self.node_amaf[x, a]) if a < self.P else (0, 0)
                u = rave_u(n, s, nt, st, lx, c, k, fpu)
                if best is None or u > best:
                    best, besta = u, int(a)
            ch = int(self.child[x, besta])
            if ch < 0:
                y = len(self.boards)
                if y > self.I:                      # no room left: x is evaluated as it is
                    return x, self.boards[x], False
                kid = c_oracle.next_state(self.boards[x], besta)
                self.boards.append(kid)
                self.legal.append(mc.legal_actions(kid))
                self.parent[y], self.action[y], self.child[x, besta] = x, besta, y
                self.max_depth = max(self.max_depth, depth + 1)
                return y, kid, True
            x, depth = ch, depth + 1

    def path(self, y):
        p = []
        while y >= 0:
            p.append(int(y))
            y = self.parent[y]
        return p[::-1]

    def backup_rave(self, y, K, bw, ww, d, amaf):
        """amaf: int [2, 3, N*N] of the leaf's playouts."""
        path = self.path(y)
        moves = [int(self.action[x]) for x in path]
        for i, x in enumerate(path):
            c = int(self.boards[x][2, 0, 0] != 0)
            S = 2 * (ww if c else bw) + d
            dn = amaf[c, 0].astype(np.int64).copy()
            ds = (2 * amaf[c, 1 + c].astype(np.int64) + amaf[c, 0] - amaf[c, 1] - amaf[c, 2]).copy()
            first = {}
            for j in range(i + 1, len(path)):
                if moves[j] < self.P:
                    first.setdefault(moves[j], j)
            for p, j in first.items():
                mine = (j - i) & 1
                dn[p], ds[p] = (K, S) if mine else (0, 0)
            self.node_amaf[x, :, 0] += dn
            self.node_amaf[x, :, 1] += ds
        self.backup(y, K, bw, ww, d)

    def update(self, y, K, e, r):
        """e: expected_playouts_amaf of the R leaves."""
        tree_pts = {int(self.action[x]) for x in self.path(y)[1:] if self.action[x] < self.P}
        if tree_pts and np.isin(e['sequences'][r * K:(r + 1) * K], list(tree_pts)).any():
            self.replayed += 1
        self.backup_rave(y, K, int(e['black_wins'][r]), int(e['white_wins'][r]), int(e['draws'][r]), e['amaf'][r].reshape(2, 3, self.P))


def expected_uct_rave(roots, I, K, c=math.sqrt(2), rave_equiv=300.0, fpu=1.0, max_plies=None, komi=0.0, base_seed=20260927, first_root=0,
                      chunk_plies=32, policy=0, iterations=None, trees=None):
    """-> dict of the outputs of batch_uct(rave_equiv=..., tree=True) (NumPy): mc_expect.run_uct's (mc_expect.ROOT_KEYS, 'tree',
    'trees') on RaveTrees, plus 'rave_visits', 'rave_score', 'node_amaf' in 'tree', and for the premises 'replayed' (per root:
    RaveTree.replayed).  iterations: how many to run on trees with room for I + 1 nodes (default I; more: a search past
    capacity).  trees: the trees to search instead of new RaveTrees (mc_prior_expect's PriorTrees)."""
    roots = np.ascontiguousarray(roots, np.uint8)
    trees = [RaveTree(root, I) for root in roots] if trees is None else trees
    out = mc.run_uct(trees, roots, I if iterations is None else iterations, K, (K, c, mc.log_table(I, K), rave_equiv, fpu),
                     functools.partial(expected_playouts_amaf, policy=policy), max_plies, komi, base_seed, first_root, chunk_plies)
    out['tree']['node_amaf'] = na = np.stack([t.node_amaf for t in trees]).astype(np.int32)
    out['rave_visits'], out['rave_score'] = na[:, 0, :, 0], na[:, 0, :, 1]
    out['replayed'] = np.array([t.replayed for t in trees], np.int64)
    return out


RAVE_ROOT_KEYS = mc.ROOT_KEYS + ('rave_visits', 'rave_score')
RAVE_TREE_KEYS = mc.TREE_KEYS + ('node_amaf',)


# ---------------------------------------------------------------- the cases of the device tests
LOG_B, LOG_PLIES = 70, (1, 7, 33)


@functools.lru_cache(maxsize=None)
def log_boards(N, B=LOG_B):
    """B boards for the log rollout: a third of them mid-game or late, three ended, the others empty."""
    named = cs.size_roots(N)
    mid = [named[k] for k in ('mid0', 'mid1', 'late0', 'late1', 'late2')]
    states = np.zeros((B, 6, N, N), np.uint8)
    for b in range(1, B, 3):
        states[b] = mid[(b // 3) % len(mid)]
    for b, k in ((5, 'ended'), (B // 2, 'played_out'), (B - 1, 'ended')):
        states[b] = named[k]
    states.setflags(write=False)
    return states


def log_seed(N, policy):
    return 4000 + 10 * N + policy


@functools.lru_cache(maxsize=None)
def log_case(N, policy, B=LOG_B, plies=max(LOG_PLIES)):
    """-> (states, generators, actions int32 [B, plies]) of the log rollout case: the launches of 1 and 7 plies play prefixes."""
    states = log_boards(N, B)
    rng = c_oracle.rng_seed(log_seed(N, policy), B)
    _, _, acts, _ = play_sequences(states, rng, plies, policy)
    return states, rng, acts


PO_K, PO_KOMI, PO_SEED = 5, 0.5, 77
PO_SIZES_MORE = (5, 9, 19)     # the sizes with slot / chunk / shard / cut-off / policy variants
PO_CUT = {5: 16, 9: 32, 19: 64}


def playout_roots(N):
    """R = 3: the empty board, a mid-game root, a finished game."""
    return cs.stack(N, ('empty', 'mid0', 'ended'))


@functools.lru_cache(maxsize=None)
def playout_case(N, policy=0, cut=False):
    """expected_playouts_amaf of the size's playout case (cut: with the max_plies of PO_CUT, which cuts playouts off)."""
    return expected_playouts_amaf(playout_roots(N), PO_K, PO_CUT[N] if cut else cs.full_cap(N), komi=PO_KOMI, base_seed=PO_SEED + N,
                                  with_ownership=True, policy=policy)


def all_playout_cases():
    """Every (N, policy, cut) the device test runs."""
    cases = [(N, 0, False) for N in SIZES]
    for N in PO_SIZES_MORE:
        cases += [(N, 0, True), (N, 1, False), (N, 2, False)]
    return cases


RAVE_SIZES = (2, 3, 5, 7, 9, 13, 19)
RAVE_I, RAVE_K, RAVE_EQUIV, RAVE_FPU, RAVE_KOMI = 24, 4, 50.0, 1.0, 0.5
RAVE_CS = (0.0, math.sqrt(2))


def rave_roots(N):
    """R = 4: a late root, a mid-game root, the empty board, a finished game."""
    return cs.stack(N, ('late0', 'mid0', 'empty', 'ended'))


@functools.lru_cache(maxsize=None)
def rave_case(N, c):
    return expected_uct_rave(rave_roots(N), RAVE_I, RAVE_K, c=c, rave_equiv=RAVE_EQUIV, fpu=RAVE_FPU, komi=RAVE_KOMI, base_seed=900 + N)


@functools.lru_cache(maxsize=None)
def plain_case(N, c):
    return mc.expected_uct(rave_roots(N), RAVE_I, RAVE_K, c=c, komi=RAVE_KOMI, base_seed=900 + N)


PAST_N, PAST_I, PAST_EXTRA = 5, 6, 4


@functools.lru_cache(maxsize=None)
def past_capacity_case():
    """A search of PAST_I + PAST_EXTRA iterations on trees with room for PAST_I + 1 nodes."""
    return expected_uct_rave(rave_roots(PAST_N), PAST_I, RAVE_K, c=0.5, rave_equiv=RAVE_EQUIV, fpu=RAVE_FPU, komi=RAVE_KOMI, base_seed=31,
                             iterations=PAST_I + PAST_EXTRA)
