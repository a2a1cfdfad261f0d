"""Expected results of the PUCT search (gogame.batch_puct / PuctSearch) and the deterministic evaluators its tests share (test
infrastructure, CPU only; builds on tests/mc_expect.py).  The search is restated in Python: expansions by the C
restatement's next_state, terminal values from its areas, U in Python floats (IEEE doubles, the operations of the
specification in its order, math.sqrt), priors and values passed through np.float32 exactly as the device takes them.

The evaluators exist twice, in NumPy (for the restatement) and in torch (for the device), and agree by construction: all
they do is int64 arithmetic without overflow on the leaf's stone planes, followed by one exact conversion (k / 256 and
m / 128 are exact in float32)."""
import math

import numpy as np

import mc_expect as mc
import mc_policy_expect as mcp
from oracle import c_oracle

ROOT_KEYS = ('legal', 'visits', 'value_sum', 'priors', 'root_visits', 'root_value_sum', 'nodes')
TREE_KEYS = ('parent', 'action', 'visits', 'value_sum')
_MUL, _ADD, _ACT = 1103515245, 12345, 2654435761


# ---------------------------------------------------------------- comparison
def bits(x):
    """float arrays as their bit patterns (so that -0.0 != 0.0 and NaN == NaN), everything else unchanged."""
    x = mc.to_np(x)
    if x.dtype == np.float64:
        return x.view(np.int64)
    if x.dtype == np.float32:
        return x.view(np.int32)
    return x


def check(got, want, tree=True, tag=''):
    """Every field of the Puct `got` equals the restatement `want` (expected_puct), floats compared as bit patterns."""
    for k in ROOT_KEYS:
        g, w = mc.to_np(getattr(got, k)), want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, k, g.shape, g.dtype, w.shape, w.dtype)
        assert np.array_equal(bits(g), bits(w)), (tag, k, np.argwhere(bits(g) != bits(w))[:8])
    if not tree:
        assert got.tree is None
        return
    for k in TREE_KEYS:
        g, w = mc.to_np(getattr(got.tree, k)), want['tree'][k]
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, 'tree', k, g.shape, g.dtype, w.shape, w.dtype)
        assert np.array_equal(bits(g), bits(w)), (tag, 'tree', k, np.argwhere(bits(g) != bits(w))[:8])


# ---------------------------------------------------------------- deterministic evaluators, NumPy and torch
def _weights(N):
    """int64 [2, N, N]: a weight below 2^20 per colour and point."""
    p = np.arange(2 * N * N, dtype=np.int64)
    return ((p * 7919 + 104729) * 31337 % (1 << 20)).reshape(2, N, N)


def _hash_np(states):
    """int64 [R] in [0, 2^31): the weighted sum of the stones (below 2^30) through one linear congruential step, and the
    turn."""
    st = np.asarray(states)
    N = st.shape[-1]
    h = ((st[:, :2] != 0).astype(np.int64) * _weights(N)[None]).reshape(st.shape[0], -1).sum(axis=1)
    h = h + (st[:, 2, 0, 0] != 0).astype(np.int64) * 977
    return (h * _MUL + _ADD) % (1 << 31)


def _hash_t(states):
    import torch
    N = states.shape[-1]
    wt = torch.from_numpy(_weights(N)).to(states.device)
    h = ((states[:, :2] != 0).to(torch.int64) * wt[None]).reshape(states.shape[0], -1).sum(dim=1)
    h = h + (states[:, 2, 0, 0] != 0).to(torch.int64) * 977
    return (h * _MUL + _ADD) % (1 << 31)


def _k_np(h, A):
    return ((h[:, None] + (np.arange(A, dtype=np.int64)[None, :] + 1) * _ACT) >> 7) % 256


def _k_t(h, A):
    import torch
    return ((h[:, None] + (torch.arange(A, dtype=torch.int64, device=h.device)[None, :] + 1) * _ACT) >> 7) % 256


def hash_evaluator_np(states, legal):
    """priors k / 256 (k in [0, 255] from the leaf's hash and the action), zero on illegal actions; values
    (h mod 257 - 128) / 128."""
    h = _hash_np(states)
    k = np.where(legal, _k_np(h, legal.shape[1]), 0)
    return k.astype(np.float32) / np.float32(256), (h % 257 - 128).astype(np.float32) / np.float32(128)


def hash_evaluator_t(states, legal):
    import torch
    h = _hash_t(states)
    k = torch.where(legal, _k_t(h, legal.shape[1]), torch.zeros((), dtype=torch.int64, device=h.device))
    return k.to(torch.float32) * 0.00390625, (h % 257 - 128).to(torch.float32) * 0.0078125   # (exact: powers of two)


def hostile_evaluator_np(states, legal):
    """The outputs a broken network gives: priors with NaN, negatives, +-inf and mass on illegal actions (nothing is masked),
    rows of all-zero priors; values three times too large, NaN and +-inf.  Which entry gets what follows from the hash."""
    h = _hash_np(states)
    k = _k_np(h, legal.shape[1])
    p = k.astype(np.float32) / np.float32(256)
    m = k % 8
    p = np.where(m == 0, np.float32(np.nan), p)
    p = np.where(m == 1, -p, p)
    p = np.where((m == 2) & (k > 200), np.float32(np.inf), p)
    p = np.where((m == 3) & (k > 200), np.float32(-np.inf), p)
    p = np.where((h % 5 == 0)[:, None], np.float32(0), p).astype(np.float32)
    v = (h % 257 - 128).astype(np.float32) * np.float32(3) / np.float32(128)
    v = np.where(h % 11 == 0, np.float32(np.nan), v)
    v = np.where(h % 13 == 0, np.float32(np.inf), v)
    v = np.where(h % 17 == 0, np.float32(-np.inf), v).astype(np.float32)
    return p, v


def hostile_evaluator_t(states, legal):
    import torch
    h = _hash_t(states)
    k = _k_t(h, legal.shape[1])
    f = lambda x: torch.full((), x, dtype=torch.float32, device=h.device)
    p = k.to(torch.float32) * 0.00390625
    m = k % 8
    p = torch.where(m == 0, f(math.nan), p)
    p = torch.where(m == 1, -p, p)
    p = torch.where((m == 2) & (k > 200), f(math.inf), p)
    p = torch.where((m == 3) & (k > 200), f(-math.inf), p)
    p = torch.where((h % 5 == 0)[:, None], f(0.0), p)
    v = (h % 257 - 128).to(torch.float32) * 3.0 * 0.0078125   # (m * 3 is an integer below 2^24: both products are exact)
    v = torch.where(h % 11 == 0, f(math.nan), v)
    v = torch.where(h % 13 == 0, f(math.inf), v)
    v = torch.where(h % 17 == 0, f(-math.inf), v)
    return p, v


def pass_evaluator_np(states, legal):
    """All the prior mass on the pass (where it is legal), the hash's values."""
    p = np.zeros(legal.shape, np.float32)
    p[:, -1] = legal[:, -1]
    return p, hash_evaluator_np(states, legal)[1]


def pass_evaluator_t(states, legal):
    import torch
    p = torch.zeros(legal.shape, dtype=torch.float32, device=legal.device)
    p[:, -1] = legal[:, -1].to(torch.float32)
    return p, hash_evaluator_t(states, legal)[1]


def playout_evaluator_np(*args, policy='uniform', **kw):
    """mc_expect.playout_evaluator_np for policy 'uniform' or 'no_eye_fill'."""
    return mc.playout_evaluator_np(*args, rollout={'uniform': None, 'no_eye_fill': mcp.policy_rollout}[policy], **kw)


# ---------------------------------------------------------------- the search
def score(s, wc, nc, prior, nx, c):
    """U of action a at node x, every operation a float64 operation in this order; a NaN counts as -inf."""
    q = 0.0 if nc == 0 else s * float(wc) / float(nc)
    t1 = float(c) * float(prior)
    t2 = math.sqrt(float(nx))
    t3 = t1 * t2
    t4 = t3 / float(1 + nc)
    u = q + t4
    return -math.inf if u != u else u


def terminal_value(board, komi):
    """sign(black area - white area - komi), komi and the difference in float32."""
    b, w = c_oracle.batch_areas(board[None])
    x = np.float32(int(b[0]) - int(w[0])) - np.float32(komi)
    return 1.0 if x > 0 else (-1.0 if x < 0 else 0.0)


class Tree:
    def __init__(self, root, I):
        N = root.shape[-1]
        A = N * N + 1
        self.I = I
        self.boards = [np.asarray(root, np.uint8)]
        self.parent = np.full(I + 1, -1, np.int32)
        self.action = np.full(I + 1, -1, np.int32)
        self.n = np.zeros(I + 1, np.int32)
        self.w = np.zeros(I + 1, np.float64)
        self.prior = np.zeros((I + 1, A), np.float32)
        self.child = np.full((I + 1, A), -1, np.int64)
        self.legal = [mc.legal_actions(self.boards[0])]
        self.evals = [[] for _ in range(I + 1)]   # per node: the values (black's point of view) of its own evaluations
        self.paths = []                           # per iteration: (leaf, move)

    def select(self, c):
        """-> (leaf id, leaf board): step 1 and the move of step 2, the new node added when there is one."""
        x = 0
        while True:
            acts = self.legal[x]
            if acts.size == 0 or self.n[x] == 0:   # the game has ended at x, or x has not been evaluated
                self.paths.append((x, -1))
                return x, self.boards[x]
            s = -1.0 if self.boards[x][2, 0, 0] != 0 else 1.0
            best, besta = None, None
            for a in acts:                         # ascending: strict > keeps the lowest action of equal scores
                k = self.child[x, a]
                nc, wc = (int(self.n[k]), float(self.w[k])) if k >= 0 else (0, 0.0)
                u = score(s, wc, nc, self.prior[x, a], int(self.n[x]), c)
                if best is None or u > best:
                    best, besta = u, int(a)
            k = int(self.child[x, besta])
            if k >= 0:
                x = k
                continue
            if len(self.boards) > self.I:          # no room (a select beyond I iterations): x is evaluated as it is
                self.paths.append((x, -1))
                return x, self.boards[x]
            y = len(self.boards)
            kid = c_oracle.next_state(self.boards[x], besta)
            self.boards.append(kid)
            self.legal.append(mc.legal_actions(kid))
            self.parent[y], self.action[y], self.child[x, besta] = x, besta, y
            self.paths.append((y, besta))
            return y, kid

    def backup(self, y, priors, value, komi):
        board = self.boards[y]
        if self.n[y] == 0:
            ok = np.zeros(self.prior.shape[1], bool)
            ok[self.legal[y]] = True
            p = np.asarray(priors, np.float32)
            with np.errstate(invalid='ignore'):
                self.prior[y] = np.where(ok & (p > 0), p, np.float32(0))
        if self.legal[y].size == 0:
            vb = terminal_value(board, komi)
        else:
            v = np.float32(value)
            v = np.float32(0) if v != v else min(max(v, np.float32(-1)), np.float32(1))
            vb = (-1.0 if board[2, 0, 0] != 0 else 1.0) * float(v)
        self.evals[y].append(vb)
        while y >= 0:
            self.n[y] += 1
            self.w[y] = float(self.w[y]) + vb
            y = self.parent[y]


def expected_puct(roots, I, evaluator_np, c=1.25, komi=0.0):
    """-> dict of the outputs of batch_puct(roots, I, evaluator, c, komi, tree=True) (NumPy; ROOT_KEYS, 'tree': dict of
    TREE_KEYS arrays [R, I + 1], 'trees': the Tree objects).  evaluator_np(states uint8 [R, 6, N, N], legal bool [R, A]) ->
    (priors float32 [R, A], values float32 [R])."""
    roots = np.ascontiguousarray(roots, np.uint8)
    R, _, N, _ = roots.shape
    A = N * N + 1
    trees = [Tree(roots[r], I) for r in range(R)]
    for _ in range(I):
        picked = [t.select(c) for t in trees]
        if R:
            leaves = np.stack([b for _, b in picked])
            priors, values = evaluator_np(leaves, mc.legal_mask(leaves))
            priors, values = np.asarray(priors, np.float32), np.asarray(values, np.float32)
            assert priors.shape == (R, A) and values.shape == (R,)
        for r, t in enumerate(trees):
            t.backup(picked[r][0], priors[r], values[r], komi)
    out = {'legal': mc.legal_mask(roots) if R else np.zeros((0, A), bool),
           'visits': np.zeros((R, A), np.int32), 'value_sum': np.zeros((R, A), np.float64),
           'priors': np.zeros((R, A), np.float32)}
    for r, t in enumerate(trees):
        has = t.child[0] >= 0
        out['visits'][r, has] = t.n[t.child[0, has]]
        out['value_sum'][r, has] = t.w[t.child[0, has]]
        out['priors'][r] = t.prior[0]
    out['root_visits'] = np.array([t.n[0] for t in trees], np.int32)
    out['root_value_sum'] = np.array([t.w[0] for t in trees], np.float64)
    out['nodes'] = np.array([len(t.boards) for t in trees], np.int32)
    stack = lambda f, dt: np.stack([f(t) for t in trees]).astype(dt) if R else np.zeros((0, I + 1), dt)
    out['tree'] = {'parent': stack(lambda t: t.parent, np.int32), 'action': stack(lambda t: t.action, np.int32),
                   'visits': stack(lambda t: t.n, np.int32), 'value_sum': stack(lambda t: t.w, np.float64)}
    out['trees'] = trees
    return out


def most_visited(res):
    """NumPy restatement of puct_actions over results `res` (dict or Puct of NumPy arrays)."""
    return mc.most_visited(res)
