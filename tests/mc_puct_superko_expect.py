"""Expected results of positional superko at every node of a PUCT tree (gogame.PuctSearch(superko=history), batch_puct(superko=),
puct_play / puct_selfplay(superko='tree'): gg_puct_superko) - test infrastructure, CPU only.  Builds on
tests/mc_puct_expect.py, mc_puct_leaves_expect.py, mc_puct_advance_expect.py and mc_puct_selfplay_expect.py by subclassing and
wrapping: when a node is created its child positions are PLAYED (the C restatement's next_state) and compared STONE BY STONE
(hash_expect.position_key, no hashes) with the earlier positions of the game and with the node's ancestors; the forbidden
points go into plane 3 of the stored board and out of the node's legal list.  Also the NumPy statement of ONE gg_puct_superko
launch on arbitrary links / node_hash / history arrays, and the planted cases of its test."""
import functools
from types import SimpleNamespace

import numpy as np

import features_expect as fe
import hash_expect as he
import mc_expect as mc
import mc_puct_advance_expect as pa
import mc_puct_expect as pe
import mc_puct_leaves_expect as pl
import mc_puct_selfplay_expect as ps
import outcome_expect as oe
from oracle import c_oracle

CHUNK = 64            # kChainChunk of gg_hash.h: ancestors (or history entries) staged per compare


def key_of(board):
    return he.position_key(board[0], board[1])


def recreating(board, keys):
    """The board moves of `board` (candidates: empty, plane 3 clear, game not over) whose child position is in `keys`."""
    N = board.shape[-1]
    out = []
    for y, x in np.argwhere(oe.candidates(board)):
        a = int(y) * N + int(x)
        kid = c_oracle.next_state(board, a)
        if key_of(kid) in keys:
            out.append(a)
    return out


def mark(board, acts):
    """a copy of `board` with plane 3 set at the points `acts`"""
    out = np.array(board, np.uint8)
    N = out.shape[-1]
    for a in acts:
        out[3, a // N, a % N] = 1
    return out


# ---------------------------------------------------------------- the trees
class _Rule:
    """What the two tree classes share.  history: the position keys of the game so far, the current root included."""

    def _init_rule(self, history):
        self.history = set(history)
        self.marks = {}        # node -> the actions the rule took from it when it was made (node 0: by forbid_root)

    def chain_keys(self, x):
        """the positions of x and of every node above it"""
        keys = set()
        while x >= 0:
            keys.add(key_of(self.boards[x]))
            x = int(self.parent[x])
        return keys

    def ruled(self, y, kid):
        """the new node y's board with its forbidden points marked"""
        acts = recreating(kid, self.history | self.chain_keys(int(self.parent[y])))
        self.marks[y] = acts
        return mark(kid, acts) if acts else kid

    def forbid_root(self):
        """PuctSearch.forbid_repeats at node 0: the history alone"""
        acts = recreating(self.boards[0], self.history)
        self.marks[0] = sorted(set(self.marks.get(0, [])) | set(acts))
        self.boards[0] = mark(self.boards[0], acts)
        self.legal[0] = mc.legal_actions(self.boards[0])


class SuperkoTree(pe.Tree, _Rule):
    def __init__(self, root, I, history):
        pe.Tree.__init__(self, root, I)
        self._init_rule(history)

    def select(self, c):
        y, board = pe.Tree.select(self, c)
        if self.paths[-1][1] >= 0:                 # a node made now
            self.boards[y] = self.ruled(y, board)
            self.legal[y] = mc.legal_actions(self.boards[y])
        return y, self.boards[y]


class SuperkoLeavesTree(pl.LeavesTree, _Rule):
    def __init__(self, root, C, history):
        pl.LeavesTree.__init__(self, root, C)
        self._init_rule(history)

    def _walk(self, c):
        y, mv, board = pl.LeavesTree._walk(self, c)
        if mv >= 0:                                # a node made now: its board waits in pending until the backup
            board = self.pending[y] = self.ruled(y, board)
        return y, mv, board


def make_trees(roots, histories, capacity, L):
    """histories: per root the boards (or position keys) of its game so far, the root included; None = the root alone"""
    roots = np.ascontiguousarray(roots, np.uint8)
    out = []
    for r in range(roots.shape[0]):
        h = [roots[r]] if histories is None else histories[r]
        keys = [k if isinstance(k, bytes) else key_of(k) for k in h]
        out.append(SuperkoTree(roots[r], capacity - 1, keys) if L is None else SuperkoLeavesTree(roots[r], capacity - 1, keys))
    return out


def advance(tree, a):
    """pa.advance, and what the caller's loop does behind it: the new root enters the history"""
    kept = pa.advance(tree, a, pa.next_root(tree, a))
    if a != -1:
        tree.marks = {}
    tree.history.add(key_of(tree.boards[0]))
    return kept


def repeats(tree, history=()):
    """The nodes of a tree (any pe.Tree) that a board move reaches and that have exactly the stones of one of their own
    ancestors or of a position in `history` (position keys)."""
    out = []
    for y in range(1, len(tree.boards)):
        if tree.boards[y] is None or tree.action[y] < 0 or tree.action[y] >= tree.prior.shape[1] - 1:
            continue
        k, x, seen = key_of(tree.boards[y]), int(tree.parent[y]), set(history)
        while x >= 0:
            seen.add(key_of(tree.boards[x]))
            x = int(tree.parent[x])
        if k in seen:
            out.append(y)
    return out


def expected_puct(roots, histories, iterations, evaluator_np, c=1.25, komi=0.0, leaves=None, capacity=None, rule=True):
    """-> pa.results() of batch_puct(roots, iterations, evaluator, c, komi, tree=True, leaves=, capacity=, superko=history) plus
    'trees'.  rule=False: the plain search on the same tree classes' parents."""
    roots = np.ascontiguousarray(roots, np.uint8)
    NN = iterations * (leaves or 1) + 1 if capacity is None else capacity
    trees = make_trees(roots, histories, NN, leaves) if rule else pa.make_trees(roots, NN, leaves)
    if rule:
        for t in trees:
            t.forbid_root()
    pa.search_rounds(trees, iterations, leaves, evaluator_np, c, komi)
    out = pa.results(trees, roots.shape[-1] ** 2 + 1)
    out['trees'] = trees
    return out


def expected_puct_play(roots, moves, iterations, evaluator_np, c=1.25, komi=0.0, leaves=None, capacity=None, reuse=True,
                       on_move=None):
    """gogame.puct_play(.., superko='tree') restated -> (actions int64 [R, moves], final states, the trees)."""
    roots = np.ascontiguousarray(roots, np.uint8)
    R = roots.shape[0]
    NN = iterations * (leaves or 1) + 1 if capacity is None else capacity
    trees = make_trees(roots, None, NN, leaves)
    played = np.zeros((R, moves), np.int64)
    for mv in range(moves):
        for t in trees:
            t.forbid_root()
        pa.search_rounds(trees, iterations, leaves, evaluator_np, c, komi)
        acts = [pa.most_visited_root(t) for t in trees]
        played[:, mv] = acts
        kept = [advance(t, a) for t, a in zip(trees, acts)]
        if on_move is not None:
            on_move(mv, trees, acts, kept)
        if not reuse:
            trees = make_trees(np.stack([t.boards[0] for t in trees]), [sorted(t.history) for t in trees], NN, leaves)
    final = np.stack([t.boards[0] for t in trees]) if R else roots
    return played, final, trees


def expected_selfplay(roots, moves, iterations, evaluator_np, c=1.25, komi=0.0, leaves=None, capacity=None, sample_moves=0,
                      seed=20260927, first_game=0):
    """gogame.puct_selfplay(.., superko='tree', record_states=True) without noise restated -> dict of the SelfPlay fields."""
    roots = np.ascontiguousarray(roots, np.uint8)
    R, _, N, _ = roots.shape
    A = N * N + 1
    NN = iterations * (leaves or 1) + 1 if capacity is None else capacity
    trees = make_trees(roots, None, NN, leaves)
    rng = ps.seeds(R, seed, first_game)
    out = {'actions': np.full((R, moves), -1, np.int64), 'pi': np.zeros((R, moves, A), np.float32),
           'value': np.zeros((R, moves), np.float32), 'lengths': np.zeros(R, np.int32),
           'states': np.zeros((R, moves, 6, N, N), np.uint8)}
    for mv in range(moves):
        out['states'][:, mv] = np.stack([t.boards[0] for t in trees])      # (recorded before forbid_repeats marks the root)
        for t in trees:
            t.forbid_root()
        pa.search_rounds(trees, iterations, leaves, evaluator_np, c, komi)
        for r, t in enumerate(trees):
            a, out['pi'][r, mv], out['value'][r, mv], rng[r] = ps.root_policy(t, mv < sample_moves, rng[r])
            out['actions'][r, mv] = a
            out['lengths'][r] += a >= 0
            advance(t, a)
    out['final_states'] = np.stack([t.boards[0] for t in trees])
    out['outcome'] = np.array([ps.outcome(t.boards[0], komi) for t in trees], np.int8)
    out['trees'] = trees
    return out


def planes_evaluator(E):
    """An evaluator of feature planes (tests/test_gpu_symmetry_io.point_evaluator) as an evaluator of states"""
    return lambda states, legal: E(fe.batch_features(states), legal)


# ---------------------------------------------------------------- one launch, in NumPy
def chain_of(links, r, y, C):
    """The ancestors the launch visits from node y of root r: while the parent p of x satisfies 0 <= p < x, at most C steps."""
    out, x = [], int(y)
    while len(out) < C:
        p = int(links[r, x, 0])
        if not 0 <= p < x:
            break
        out.append(p)
        x = p
    return out


def launch(states, hashes, moves, move, leaf_id, links, node_hash, history, count, C, L):
    """One gg_puct_superko launch -> (rows uint32 [B, N]: what is ORed into words [2N, 3N) of every leaf, node_hash afterwards).
    states uint8 [B, 6, N, N]: the leaves; hashes int64 [B] and moves int64 [B, N*N + 1]: their position and move hashes
    (hash_expect); history int64 [R, H] and count int32 [R], or both None."""
    B, N = states.shape[0], states.shape[-1]
    P = N * N
    rows = np.zeros((B, N), np.uint32)
    out = np.array(node_hash, np.int64)
    for i in range(B):
        r, y, m = i // L, int(leaf_id[i]), int(move[i])
        if y < 1 or y > C or m < 0:
            continue
        out[r, y] = hashes[i]
        bad = set()
        if history is not None:
            bad |= {int(v) for v in history[r, :min(max(int(count[r]), 0), history.shape[1])]}
        bad |= {int(node_hash[r, x]) for x in chain_of(links, r, y, C)}
        for yy, xx in np.argwhere(oe.candidates(states[i])):
            if int(moves[i, yy * N + xx]) in bad:
                rows[i, yy] |= np.uint32(1 << int(xx))
    return rows, out


# ---------------------------------------------------------------- the planted cases of the launch test
ROOTS, SLOTS = 8, 3
C_CASE = 2 * CHUNK + 2
H_CASE = CHUNK + 6
COUNTS = (0, 1, H_CASE, H_CASE + 5, -1)
EDGES = (0, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK)      # chain positions at either side of every chunk boundary


def _pool(N):
    """Boards of size N with candidates, those with a capturing candidate first -> (states, hashes, moves, capturing [B, P])."""
    states = [np.asarray(he.case(N, k).states) for k in ('policy', 'clean')]
    caps = [np.asarray(oe.case(N, k).raw)[:, 1].reshape(len(s), -1) > 0 for k, s in zip(('policy', 'clean'), states)]
    hashes = [he.case(N, k).hashes for k in ('policy', 'clean')]
    moves = [he.case(N, k).moves for k in ('policy', 'clean')]
    if N in he.GAME_SEEDS:                          # the positions of real games, where captures are the rule
        g = he.games(N).states.reshape((-1, 6, N, N))
        _, first = np.unique(g.reshape(len(g), -1), axis=0, return_index=True)
        g = g[np.sort(first)][:96]
        cap = np.zeros((len(g), N * N), bool)
        for b, s in enumerate(g):
            for y, x in np.argwhere(oe.candidates(s)):
                cap[b, y * N + x] = he.child(s, int(y), int(x))[2] > 0
        states.append(g); caps.append(cap); hashes.append(he.batch_hash(g)); moves.append(he.batch_move_hashes(g))
    states, caps, hashes, moves = (np.concatenate(v) for v in (states, caps, hashes, moves))
    cand = oe.candidates_of(states).reshape(len(states), -1)
    caps = caps & cand
    order = np.lexsort((-cand.sum(axis=1), -(caps.any(axis=1)).astype(int)))
    order = [b for b in order if cand[b].any()]
    return states[order], hashes[order], moves[order], caps[order]


def depth_plan(N):
    """The chain depths of the marked rows of size N: 1, C, both sides of the chunk boundaries, and this size's share of all the
    others (the 18 sizes together cover every depth from 1 to C)."""
    fixed = [C_CASE, 1, 2 * CHUNK + 1, 2 * CHUNK, CHUNK, CHUNK + 1]    # (C: root 0's only marked row; C - 1: a root of two)
    rest = [d for d in range(2, C_CASE) if d not in fixed]
    return fixed + rest[(N - 2)::18]


@functools.lru_cache(maxsize=None)
def planted(N):
    """The launch test's case of size N, read only: 8 roots x 3 rows on C = 2 * chunk + 2.  .states / .hashes / .moves of the 24
    leaves, .move / .leaf_id, .links, .node_hash, .history / .count, .rows and .node_hash_after (the expectation), and what was
    planted: .hits [(row, action, where)], .decoys [(row, action, where)], .depths {row: depth}, .untouched rows."""
    rs = np.random.RandomState(1000 + N)
    C, L, R, H, P = C_CASE, SLOTS, ROOTS, H_CASE, N * N
    B = R * L
    pool_s, pool_h, pool_m, pool_c = _pool(N)
    pick = np.arange(B) % len(pool_s)
    states, hashes, moves, caps = pool_s[pick], pool_h[pick], pool_m[pick], pool_c[pick]
    rnd = lambda *shape: rs.randint(-2 ** 62, 2 ** 62, size=shape, dtype=np.int64) * 2 + 1   # (odd: never a planted hash by design)
    links = np.full((R, C + 1, 2), -1, np.int32)
    for x in range(1, C + 1):
        links[:, x, 0] = rs.randint(0, x, size=R)                 # random descending parents everywhere
        links[:, x, 1] = rs.randint(0, P + 1, size=R)
    node_hash = rnd(R, C + 1)
    history = rnd(R, H)
    count = np.array([COUNTS[r % len(COUNTS)] for r in range(R)], np.int32)
    move = rs.randint(0, P, size=B).astype(np.int32)
    leaf_id = np.zeros(B, np.int32)
    untouched = {0 * L + 1: 'leaf_id = -1', 0 * L + 2: 'move = -1', 1 * L + 1: 'leaf_id = 0', 2 * L + 2: 'leaf_id = C + 1'}
    leaf_id[0 * L + 1] = -1
    leaf_id[0 * L + 2], move[0 * L + 2] = 5, -1
    leaf_id[1 * L + 1] = 0
    leaf_id[2 * L + 2] = C + 1
    marked = [i for i in range(B) if i not in untouched]
    plan = depth_plan(N)
    depths, chains = {}, {}
    for r in range(R):
        mine = [i for i in marked if i // L == r]
        want = [plan.pop(0) if plan else int(rs.randint(1, C - 4)) for _ in mine]
        # the shallowest row takes the highest node, so that the deepest has every node below it for its chain; a chain never
        # passes through another row's leaf (a node made in the same round)
        ys, taken = {}, set()
        for k, (i, d) in enumerate(sorted(zip(mine, want), key=lambda t: t[1])):
            ys[i], depths[i] = C - k, d
            taken.add(C - k)
        deepest = max(mine, key=lambda i: depths[i])
        for i in sorted(mine, key=lambda i: -depths[i]):
            y, d = ys[i], depths[i]
            if i == deepest:
                free = [x for x in range(1, y) if x not in taken]
                assert len(free) >= d - 1, (N, r, y, d)
                mid = sorted(rs.choice(free, size=d - 1, replace=False).tolist(), reverse=True) if d > 1 else []
                chain = mid + [0]
                for x, p in zip(chain[:-1], chain[1:]):
                    links[r, x, 0] = p
            else:                               # the root's other rows hang off the deepest chain, as deep as they are meant to be
                chain = chains[deepest][-d:]
            links[r, y, 0] = chain[0]
            leaf_id[i], chains[i] = y, chain
    hits, decoys = [], []
    used = [dict() for _ in range(R)]       # per root: the planted places ('node', x) / ('history', e) -> the hash put there
    cands = {}
    for i in marked:
        r, chain = i // L, chains[i]
        assert chain_of(links, r, leaf_id[i], C) == chain and len(chain) == depths[i]
        cand = np.flatnonzero(oe.candidates(states[i]).reshape(-1))
        cand = [int(a) for a in cand if np.count_nonzero(moves[i, cand] == moves[i, a]) == 1]     # (a hash names one candidate)
        cand.sort(key=lambda a: not caps[i, a])                                                      # capturing candidates first
        cands[i] = cand
        n = min(max(int(count[r]), 0), H)
        spots = [('chain', k) for k in sorted({0, len(chain) - 1} | {e for e in EDGES if e < len(chain)})]
        spots += [('history', e) for e in (0, CHUNK - 1, CHUNK, H - 1) if e < n]
        turn = 0
        for where in spots:
            place = ('node', chain[where[1]]) if where[0] == 'chain' else where
            if len(cand) < 2 or place in used[r]:      # (node 0 and the history are shared by the root's rows: first come)
                continue
            a = cand[turn % (len(cand) - 1)]           # (the last candidate is kept for the decoys)
            turn += 1
            used[r][place] = int(moves[i, a])
            if where[0] == 'chain':
                node_hash[r, place[1]] = moves[i, a]
            else:
                history[r, where[1]] = moves[i, a]
            hits.append((i, a, where))
    # the decoys, once every hit stands: a candidate whose hash is planted nowhere in its root, put where it must not count
    for i in marked:
        r, cand = i // L, cands[i]
        if len(cand) < 2 or int(moves[i, cand[-1]]) in used[r].values():
            continue
        a, q, n = cand[-1], (i // L + 1) % R, min(max(int(count[r]), 0), H)
        busy = lambda root: ({x for k in marked if k // L == root for x in chains[k]} | {int(leaf_id[k]) for k in marked if k // L == root}
                             | {pl[1] for pl in used[root] if pl[0] == 'node'})
        off = [x for x in range(1, C + 1) if x not in busy(r)]
        if off:                                 # (root 0's chain of depth C leaves no node off it)
            x = off[(7 * i) % len(off)]
            node_hash[r, x] = moves[i, a]
            decoys.append((i, a, ('off-chain', x)))
        if n < H and ('history', n) not in used[r]:
            history[r, n] = moves[i, a]
            decoys.append((i, a, ('beyond count', n)))
        off = [x for x in range(C, 0, -1) if x not in busy(q)]
        if off:
            x = off[(3 * i) % len(off)]
            node_hash[q, x] = moves[i, a]
            decoys.append((i, a, ('other root', q, x)))
    rows, after = launch(states, hashes, moves, move, leaf_id, links, node_hash, history, count, C, L)
    c = SimpleNamespace(N=N, C=C, L=L, R=R, H=H, states=states, hashes=hashes, moves=moves, move=move, leaf_id=leaf_id, links=links,
                        node_hash=node_hash, history=history, count=count, rows=rows, node_hash_after=after, hits=hits,
                        decoys=decoys, depths=depths, chains=chains, untouched=untouched, marked=marked, caps=caps)
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c
