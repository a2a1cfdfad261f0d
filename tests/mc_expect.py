"""Expected results of the Monte Carlo stack (gogame.batch_playouts, batch_move_playouts, batch_uct) and the helpers its
tests share, built from the C restatement under oracle/ (test infrastructure, CPU only).  Every playout is replayed whole
(its job's generator, auto_reset off), scored with the restatement's areas and reduced on the host (replay); first moves
and tree expansions are played by the restatement's next_state; the search itself is restated in Python (Tree: U in Python
floats - IEEE doubles, the same operations in the same order, math.sqrt).

Each restatement exists once.  What a playout policy changes is the rollout that plays the playouts: replay, expected_playouts,
expected_move_playouts, expected_uct and playout_evaluator_np take it as `rollout` - None: the uniform playouts, played by the C
restatement; else a Python rollout of the policy modules (mc_policy_expect.policy_rollout's shape).  What a search mode changes
is its tree class (Tree here, RaveTree in mc_amaf_expect, PriorTree in mc_prior_expect): run_uct drives any of them and packs
the result."""
import functools
import math

import numpy as np
from scipy import ndimage

from oracle import c_oracle

GOLDEN_GAMMA = 0x9E3779B97F4A7C15   # splitmix64 increment: the sampler adds it to the generator once per ply
GAMMA_INV = pow(GOLDEN_GAMMA, -1, 2 ** 64)
JOB_MUL = 0xD1342543DE82EF95        # job id multiplier of the seeding
KEYS = ('black_wins', 'white_wins', 'draws', 'unfinished', 'margin_sum', 'plies_sum')
ROOT_KEYS = ('legal', 'visits', 'black_wins', 'white_wins', 'draws', 'root_visits', 'unfinished', 'plies_sum', 'nodes')
TREE_KEYS = ('parent', 'action', 'visits', 'black_wins', 'white_wins', 'draws')


# ---------------------------------------------------------------- what the GPU tests share
def to_np(t):
    return t.cpu().numpy() if hasattr(t, 'cpu') else np.asarray(t)


def to_dev(roots):
    import torch
    return torch.from_numpy(np.ascontiguousarray(roots)).cuda()


def check(got, want, fields, tag=''):
    """Every field of `got` (a namedtuple of tensors or arrays) has the shape and the values of want[field]."""
    for k in fields:
        g = to_np(getattr(got, k))
        assert g.shape == want[k].shape, (tag, k, g.shape, want[k].shape)
        assert np.array_equal(g, want[k]), (tag, k, np.argwhere(g != want[k])[:8])


# ---------------------------------------------------------------- generators, replay, choice
def po_seed(base_seed, p):
    """Generator of global job p (po_seed of gg_po.h, gg_rng_seed(base_seed, first_game = p)): splitmix64's state after one
    step from base_seed ^ p * JOB_MUL, mod 2^64.  p: int or integer array -> uint64 array."""
    p = np.asarray(p, dtype=np.int64).astype(np.uint64)
    with np.errstate(over='ignore'):
        return (np.uint64(base_seed & (2 ** 64 - 1)) ^ (p * np.uint64(JOB_MUL))) + np.uint64(GOLDEN_GAMMA)



def plies_from_rng(rng_before, rng_after):
    """Plies a playout played: the sampler adds GOLDEN_GAMMA to the generator once per ply, so (after - before) / GOLDEN_GAMMA
    mod 2^64."""
    d = np.asarray(rng_after, np.uint64) - np.asarray(rng_before, np.uint64)
    return (d * np.uint64(GAMMA_INV)).astype(np.int64)


def ownership(states):
    """Per point of each board [B, 6, N, N] -> uint8 [B, 2, N, N]: in black's / white's Tromp-Taylor area (a stone of that
    colour, or an empty region - 4-connected - that touches only that colour)."""
    B, _, N, _ = states.shape
    out = np.zeros((B, 2, N, N), np.uint8)
    for i in range(B):
        bl, wh = states[i, 0] != 0, states[i, 1] != 0
        empty = ~(bl | wh)
        lab, n = ndimage.label(empty)
        touch = []
        for col in (bl, wh):
            adj = np.zeros_like(col)
            adj[1:] |= col[:-1]
            adj[:-1] |= col[1:]
            adj[:, 1:] |= col[:, :-1]
            adj[:, :-1] |= col[:, 1:]
            t = np.zeros(n + 1, bool)
            t[lab[adj & empty]] = True
            t[0] = False
            touch.append(t[lab])
        out[i, 0] = bl | (touch[0] & ~touch[1])
        out[i, 1] = wh | (touch[1] & ~touch[0])
    return out



def replay(starts, jobs, K, max_plies, komi, base_seed, with_ownership=False, rollout=None):
    """K playouts from each of the G boards `starts` ([G, 6, N, N]); playout j of board g is global job jobs[g * K + j].
    -> dict of KEYS (int64 [G]) and 'ownership' (int32 [G, 2, N, N] or None).  rollout: see the module's docstring; the plies
    a Python rollout counts must be those its generators moved by."""
    G, _, N, _ = starts.shape
    rng0 = po_seed(base_seed, jobs)
    if rollout is None:
        fin, rng1, _ = c_oracle.batch_rollout_mt(np.repeat(starts, K, axis=0), rng0.copy(), max_plies, auto_reset=False)
    else:
        fin, rng1, _, steps = rollout(np.repeat(starts, K, axis=0), rng0.copy(), max_plies, auto_reset=False)
        assert np.array_equal(plies_from_rng(rng0, rng1), steps)
    b, w = c_oracle.batch_areas_mt(fin)
    d = np.asarray(b, np.int64) - np.asarray(w, np.int64)
    x = d - komi
    ended = fin[:, 5, 0, 0] != 0
    per = lambda v: np.asarray(v, np.int64).reshape(G, K).sum(axis=1)
    out = {'black_wins': per(x > 0), 'white_wins': per(x < 0), 'draws': per(x == 0), 'unfinished': per(~ended),
           'margin_sum': per(d), 'plies_sum': per(plies_from_rng(rng0, rng1)), 'ownership': None}
    if with_ownership:
        out['ownership'] = ownership(fin).astype(np.int32).reshape(G, K, 2, N, N).sum(axis=1).astype(np.int32)
    return out


def legal_mask(roots):
    """bool [R, N*N + 1]: valid_moves (plane 3 clear, pass always) of every root, all False for a root whose game has ended."""
    roots = np.asarray(roots)
    R, _, N, _ = roots.shape
    valid = np.concatenate([roots[:, 3].reshape(R, N * N) == 0, np.ones((R, 1), bool)], axis=1)
    ended = roots[:, 5].reshape(R, -1).any(axis=1)
    valid[ended] = False
    return valid



def best_legal(legal, score):
    """Per row, the legal action with the largest score (int64), ties to the lowest action, -1 without a legal action."""
    out = np.full(legal.shape[0], -1, np.int64)
    for i in range(legal.shape[0]):
        if legal[i].any():
            s = np.where(legal[i], score[i], np.iinfo(np.int64).min)
            out[i] = int(np.flatnonzero(s == s.max())[0])
    return out


def _getter(res):
    return (lambda k: np.asarray(res[k])) if isinstance(res, dict) else (lambda k: np.asarray(getattr(res, k)))


def flat_mc_choice(roots, res):
    """NumPy restatement of flat_mc_actions over results `res` (dict or MovePlayouts of NumPy arrays)."""
    get = _getter(res)
    bw, ww = get('black_wins').astype(np.int64), get('white_wins').astype(np.int64)
    white = np.asarray(roots)[:, 2, 0, 0] != 0
    return best_legal(get('legal').astype(bool), np.where(white[:, None], ww - bw, bw - ww))


def most_visited(res):
    """NumPy restatement of uct_actions over results `res` (dict or Uct of NumPy arrays)."""
    get = _getter(res)
    return best_legal(get('legal').astype(bool), get('visits').astype(np.int64))


# ---------------------------------------------------------------- batch_playouts
def expected_playouts(roots, K, max_plies, komi=0.0, base_seed=20260927, first_root=0, with_ownership=False, rollout=None):
    """-> dict of the per-root outputs of batch_playouts (NumPy), every playout replayed by the restatement."""
    roots = np.ascontiguousarray(roots, np.uint8)
    R = roots.shape[0]
    out = replay(roots, first_root * K + np.arange(R * K), K, max_plies, komi, base_seed, with_ownership, rollout)
    for k in KEYS[:4]:
        out[k] = out[k].astype(np.int32)
    return out


# ---------------------------------------------------------------- batch_move_playouts
def children_of(roots, legal):
    """The children of the legal pairs in row-major (root, action) order -> (r, a, children uint8 [T, 6, N, N])."""
    r, a = np.nonzero(legal)
    kids, status = c_oracle.batch_next_states(np.ascontiguousarray(roots, np.uint8)[r], a.astype(np.int32))
    assert not status.any()
    return r, a, kids



def expected_move_playouts(roots, K, max_plies, komi=0.0, base_seed=20260927, first_root=0, rollout=None):
    """-> dict of the outputs of batch_move_playouts ([R, A] NumPy arrays, legal included): every legal first move (whatever
    the policy makes of it), every playout after it replayed."""
    roots = np.ascontiguousarray(roots, np.uint8)
    R, _, N, _ = roots.shape
    A = N * N + 1
    legal = legal_mask(roots)
    out = {'legal': legal}
    for k in KEYS:
        out[k] = np.zeros((R, A), np.int32 if k not in ('margin_sum', 'plies_sum') else np.int64)
    if not legal.any():
        return out
    r, a, kids = children_of(roots, legal)
    jobs = (((first_root + r) * A + a)[:, None] * K + np.arange(K)[None, :]).reshape(-1)
    vals = replay(kids, jobs, K, max_plies, komi, base_seed, rollout=rollout)
    for k in KEYS:
        out[k][r, a] = vals[k]
    return out


# ---------------------------------------------------------------- batch_uct
def log_table(I, K):
    """L[t] = log(t K), t = 0 .. I, float64 by NumPy (the table the host passes to the device)."""
    with np.errstate(divide='ignore'):
        return np.log(np.arange(I + 1, dtype=np.float64) * K)


def legal_actions(board):
    """Legal actions of a node (uint8 [6, N, N]), ascending: none once the game has ended, else the points whose plane-3 bit
    is clear and the pass."""
    return np.flatnonzero(legal_mask(board[None])[0])


def score(w, d, n, log_nx, c):
    """U of a child: (2 w + d) / (2 n) + c * sqrt(log_nx / n), each operation a float64 operation in this order."""
    return (2.0 * float(w) + float(d)) / (2.0 * float(n)) + float(c) * math.sqrt(float(log_nx) / float(n))


class Tree:
    def __init__(self, root, I):
        N = root.shape[-1]
        A = N * N + 1
        self.boards = [np.asarray(root, np.uint8)]
        self.parent = np.full(I + 1, -1, np.int32)
        self.action = np.full(I + 1, -1, np.int32)
        self.stats = np.zeros((I + 1, 4), np.int64)   # n, black wins, white wins, draws
        self.child = np.full((I + 1, A), -1, np.int64)
        self.legal = [legal_actions(self.boards[0])]

    def select(self, K, c, L):
        """-> (leaf id, leaf board): step 1 of an iteration, the new node added when there is one."""
        x = 0
        while True:
            acts = self.legal[x]
            if acts.size == 0:                     # the game has ended at x
                return x, self.boards[x]
            free = acts[self.child[x, acts] < 0]
            if free.size:                          # expand the lowest legal action without a child
                a = int(free[0])
                y = len(self.boards)
                kid = c_oracle.next_state(self.boards[x], a)
                self.boards.append(kid)
                self.legal.append(legal_actions(kid))
                self.parent[y], self.action[y], self.child[x, a] = x, a, y
                return y, kid
            white = self.boards[x][2, 0, 0] != 0
            lx = L[self.stats[x, 0] // K]
            best, besta = None, None
            for a in acts:                         # ascending: strict > keeps the lowest action of equal scores
                n, bw, ww, d = self.stats[self.child[x, a]]
                u = score(ww if white else bw, d, n, lx, c)
                if best is None or u > best:
                    best, besta = u, a
            x = int(self.child[x, besta])

    def backup(self, y, K, bw, ww, d):
        while y >= 0:
            self.stats[y] += (K, bw, ww, d)
            y = self.parent[y]

    def update(self, y, K, e, r):
        """Step 3 of an iteration: the results e (of the R leaves' playouts) of this tree's leaf y, the tree of root r."""
        self.backup(y, K, e['black_wins'][r], e['white_wins'][r], e['draws'][r])


def run_uct(trees, roots, iterations, K, sel, playouts, max_plies, komi, base_seed, first_root, chunk_plies):
    """The search over one tree per root, whatever the tree class: `iterations` times select a leaf per tree (t.select(*sel) ->
    (leaf id, leaf board, ..)), evaluate the R leaves (playouts: expected_playouts or a function of its shape), update every
    tree (t.update).  -> dict of the outputs of batch_uct (NumPy; ROOT_KEYS, 'tree': dict of TREE_KEYS arrays [R, nodes]) and
    'trees'."""
    R, _, N, _ = roots.shape
    A = N * N + 1
    if max_plies is None:
        max_plies = -(-8 * N * N // chunk_plies) * chunk_plies
    unfinished = np.zeros(R, np.int64)
    plies = np.zeros(R, np.int64)
    for i in range(iterations):
        picked = [t.select(*sel) for t in trees]
        leaves = np.stack([p[1] for p in picked])
        e = playouts(leaves, K, max_plies, komi=komi, base_seed=int(po_seed(base_seed, i)), first_root=first_root)
        for r, t in enumerate(trees):
            t.update(picked[r][0], K, e, r)
        unfinished += e['unfinished']
        plies += e['plies_sum']
    out = {'legal': legal_mask(roots)}
    for k in ('visits', 'black_wins', 'white_wins', 'draws'):
        out[k] = np.zeros((R, A), np.int32)
    for r, t in enumerate(trees):
        has = t.child[0] >= 0
        for j, k in enumerate(('visits', 'black_wins', 'white_wins', 'draws')):
            out[k][r, has] = t.stats[t.child[0, has], j]
    out['root_visits'] = np.array([t.stats[0, 0] for t in trees], np.int32)
    out['unfinished'] = unfinished
    out['plies_sum'] = plies
    out['nodes'] = np.array([len(t.boards) for t in trees], np.int32)
    tree = {'parent': np.stack([t.parent for t in trees]), 'action': np.stack([t.action for t in trees])}
    for j, k in enumerate(('visits', 'black_wins', 'white_wins', 'draws')):
        tree[k] = np.stack([t.stats[:, j] for t in trees]).astype(np.int32)
    out['tree'] = tree
    out['trees'] = trees
    return out


def expected_uct(roots, I, K, c=math.sqrt(2), max_plies=None, komi=0.0, base_seed=20260927, first_root=0, chunk_plies=32,
                 rollout=None):
    """-> run_uct's dict of the outputs of batch_uct, the leaves evaluated by expected_playouts (the tree keeps every legal
    action, whatever the rollout)."""
    roots = np.ascontiguousarray(roots, np.uint8)
    return run_uct([Tree(root, I) for root in roots], roots, I, K, (K, c, log_table(I, K)),
                   functools.partial(expected_playouts, rollout=rollout), max_plies, komi, base_seed, first_root, chunk_plies)


def playout_evaluator_np(K, max_plies, komi=0.0, seed=20260927, first_root=0, rollout=None):
    """The restatement of gogame.playout_evaluator (the evaluator of a PUCT search, mc_puct_expect): call j replays
    batch_playouts(leaves, K, max_plies, komi, seed=po_seed(seed, j), first_root, policy=the rollout's) - uniform priors over
    the legal actions, (the mover's wins - losses) / K."""
    calls = [0]

    def evaluate(states, legal):
        j = calls[0]
        calls[0] += 1
        e = expected_playouts(states, K, max_plies, komi=komi, base_seed=int(po_seed(seed, j)), first_root=first_root, rollout=rollout)
        with np.errstate(divide='ignore'):
            p = np.where(legal, np.float32(1) / legal.sum(axis=1, keepdims=True).astype(np.float32), np.float32(0))
        d = e['black_wins'].astype(np.int32) - e['white_wins'].astype(np.int32)
        white = np.asarray(states)[:, 2, 0, 0] != 0
        return p.astype(np.float32), np.where(white, -d, d).astype(np.float32) / np.float32(K)

    return evaluate


# ---------------------------------------------------------------- roots
def make_roots(N, R, seed, max_ply=200, step=8):
    """R positions of random play from the empty board, root r after (r * step) % (max_ply + step) plies (r = 0: the empty
    board), plus - as the last root - a game played to its end."""
    roots = np.zeros((R, 6, N, N), np.uint8)
    target = (np.arange(R) * step) % (max_ply + step)
    rng = c_oracle.rng_seed(seed, R)
    for t in range(0, int(target.max()), step):
        m = target > t
        roots[m], rng[m], _ = c_oracle.batch_rollout(roots[m], rng[m], step, auto_reset=False)
    end, _, _ = c_oracle.batch_rollout(np.zeros((1, 6, N, N), np.uint8), c_oracle.rng_seed(seed + 1, 1), 8 * N * N + 64,
                                       auto_reset=False)
    assert end[0, 5, 0, 0] == 1
    roots[-1] = end[0]
    return roots


KO_POINT = (1, 1)


def crafted_roots(N):
    """Hand-made roots of size N >= 4 (3 has no room for the ko shape): [the empty board, a root whose last move was a pass (its pass child is terminal), a
    root with an active ko point at KO_POINT (white to move may not retake), a finished game]."""
    empty = np.zeros((6, N, N), np.uint8)
    passed = c_oracle.next_state(c_oracle.next_state(empty, (N // 2) * N + N // 2), N * N)   # black plays, white passes
    # black surrounds (1, 1) on three sides, white surrounds (1, 2); white plays into (1, 1), black captures it from (1, 2)
    ko = empty
    for y, x in [(0, 1), (0, 2), (1, 0), (1, 3), (2, 1), (2, 2), (N - 1, N - 1), (1, 1), (1, 2)]:
        ko = c_oracle.next_state(ko, y * N + x)
    assert ko[1, 1, 1] == 0 and ko[0, 1, 2] == 1 and ko[3, 1, 1] == 1 and ko[2].all()
    end = c_oracle.next_state(c_oracle.next_state(empty, N * N), N * N)
    assert passed[4].all() and not passed[5].any() and end[5].all()
    return np.stack([empty, passed, ko, end])


CAPTURE_ROWS = ('WWWWWW.',   # the white group on top has one liberty, (0, 6); black's row below it one too, (1, 6)
                'BBBBBB.',
                'WWWWWWW',
                '.......',
                'BBBBBBB',
                '.......',
                '.......')
CAPTURE_MOVE = 6             # black to move: (0, 6) captures the top group and wins the race


def capture_root():
    """A 7x7 root, black to move, where one move (CAPTURE_MOVE) captures a large group and decides the game."""
    N = len(CAPTURE_ROWS)
    st = np.zeros((6, N, N), np.uint8)
    for y, row in enumerate(CAPTURE_ROWS):
        for x, c in enumerate(row):
            st[0 if c == 'B' else 1, y, x] = c != '.'
    st[3] = c_oracle.compute_invalid_moves(st, 0)
    return st
