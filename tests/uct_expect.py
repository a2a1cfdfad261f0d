"""Expected results of gogame.batch_uct (UCT tree search), built from the C restatement under oracle/ (test infrastructure,
CPU only): the same search in Python - expansion by the restatement's next_state, U in Python floats (IEEE doubles, the
same operations in the same order, math.sqrt), and every iteration's leaves evaluated by playout_expect.expected, which
replays every playout."""
import math

import numpy as np

from oracle import c_oracle
import playout_expect as px
import move_playout_expect as mx

ROOT_KEYS = ('legal', 'visits', 'black_wins', 'white_wins', 'draws', 'root_visits', 'unfinished', 'plies_sum', 'nodes')
TREE_KEYS = ('parent', 'action', 'visits', 'black_wins', 'white_wins', 'draws')


def iteration_seed(base_seed, i):
    """Base seed of iteration i's playouts: the value gg_rng_seed(base_seed, first_game = i) writes."""
    return int(c_oracle.rng_seed(base_seed, i + 1)[i])


def log_table(I, K):
    """L[t] = log(t K), t = 0 .. I, float64 by NumPy (the table the host passes to the device)."""
    with np.errstate(divide='ignore'):
        return np.log(np.arange(I + 1, dtype=np.float64) * K)


def legal_actions(board):
    """Legal actions of a node (uint8 [6, N, N]), ascending: none once the game has ended, else the points whose plane-3 bit
    is clear and the pass."""
    return np.flatnonzero(mx.legal_mask(board[None])[0])


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


def expected(roots, I, K, c=math.sqrt(2), max_plies=None, komi=0.0, base_seed=20260927, first_root=0, chunk_plies=32):
    """-> dict of the outputs of batch_uct (NumPy; ROOT_KEYS, plus 'tree': dict of TREE_KEYS arrays [R, I + 1])."""
    roots = np.ascontiguousarray(roots, np.uint8)
    R, _, N, _ = roots.shape
    A = N * N + 1
    if max_plies is None:
        max_plies = -(-8 * N * N // chunk_plies) * chunk_plies
    L = log_table(I, K)
    trees = [Tree(roots[r], I) for r in range(R)]
    unfinished = np.zeros(R, np.int64)
    plies = np.zeros(R, np.int64)
    for i in range(I):
        picked = [t.select(K, c, L) for t in trees]
        leaves = np.stack([b for _, b in picked])
        e = px.expected(leaves, K, max_plies, komi=komi, base_seed=iteration_seed(base_seed, i), first_root=first_root)
        for r, t in enumerate(trees):
            t.backup(picked[r][0], K, e['black_wins'][r], e['white_wins'][r], e['draws'][r])
        unfinished += e['unfinished']
        plies += e['plies_sum']
    out = {'legal': mx.legal_mask(roots)}
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


def most_visited(res):
    """NumPy restatement of uct_actions over results `res` (dict or Uct of NumPy arrays)."""
    get = (lambda k: res[k]) if isinstance(res, dict) else (lambda k: getattr(res, k))
    legal = np.asarray(get('legal'), bool)
    v = np.where(legal, np.asarray(get('visits'), np.int64), -1)
    out = np.full(legal.shape[0], -1, np.int64)
    for i in range(legal.shape[0]):
        if legal[i].any():
            out[i] = int(np.flatnonzero(v[i] == v[i].max())[0])
    return out
