"""Expected results of tree reuse across moves (gogame.PuctSearch.advance / puct_play: gg_puct_advance) - test infrastructure,
CPU only.  Builds on tests/mc_puct_expect.py and tests/mc_puct_leaves_expect.py: advance() re-roots a Tree / LeavesTree in
place, written from the text of include/gymgo_amd.h (the kept set by one ascending pass over the parents, the
order-preserving renumbering, begin's state for everything behind it); expected_puct_play() is the move loop of
gogame.puct_play.  The next boards come from the C restatement's next_state."""
import numpy as np

import mc_expect as mc
import mc_puct_expect as pe
import mc_puct_leaves_expect as pl
from oracle import c_oracle


def subtree(tree, k):
    """The ids of k and of every node below it, found from the child tables (not from the parents, as advance does)."""
    out, todo = [], [int(k)]
    while todo:
        x = todo.pop()
        out.append(x)
        todo.extend(int(c) for c in tree.child[x] if c >= 0)
    return sorted(out)


def advance(tree, a, next_board):
    """Play action a at the root of `tree` (pe.Tree or pl.LeavesTree, outside a round) -> kept.  a = -1: nothing changes,
    kept = the nodes in use.  A root child under a: its subtree becomes the tree, kept = its size.  Anything else: the fresh
    tree on next_board (uint8 [6, N, N]: what the caller's game makes of the root and a), kept = 0.  tree.zeroed, the end of
    the nodes whose boards an advance has set to zero, is kept for the tests that compare the whole board buffer."""
    m = len(tree.boards)
    A = tree.prior.shape[1]
    assert not getattr(tree, 'pending', None) and not getattr(tree, 'v', np.zeros(1)).any()
    if a == -1:
        return m
    tree.zeroed = max(getattr(tree, 'zeroed', 0), m)
    k = int(tree.child[0, a]) if 0 <= a < A else -1
    if not 1 <= k < m:
        k = -1
    new = np.full(m, -1, np.int64)
    if k > 0:
        count = 0
        for x in range(k, m):                               # ascending: parents have smaller ids
            p = int(tree.parent[x])
            if x == k or (k <= p < x and new[p] >= 0):
                new[x] = count
                count += 1
    kept = [x for x in range(m) if new[x] >= 0]
    boards, legal, evals = [tree.boards[x] for x in kept], [tree.legal[x] for x in kept], [tree.evals[x] for x in kept]
    rows = {name: getattr(tree, name)[kept].copy() for name in ('parent', 'action', 'n', 'w', 'prior', 'child')}
    for name, fill in (('parent', -1), ('action', -1), ('n', 0), ('w', 0.0), ('prior', np.float32(0)), ('child', -1)):
        arr = getattr(tree, name)
        arr[:m] = fill                                      # begin's state for every node in use; nodes >= m are not touched
        arr[:len(kept)] = rows[name]
    for j, x in enumerate(kept):
        p = int(tree.parent[j])
        tree.parent[j], tree.action[j] = (-1, -1) if x == k else (new[p], tree.action[j])
        row = tree.child[j]
        inside = (row > x) & (row < m)
        row[inside] = new[row[inside]]
        row[(row >= 0) & ~inside] = -1
    if hasattr(tree, 'v'):
        tree.v[:m] = 0
    if k < 0:
        boards, legal, evals = [np.asarray(next_board, np.uint8)], [mc.legal_actions(np.asarray(next_board, np.uint8))], [[]]
    tree.boards, tree.legal = boards, legal
    tree.evals = evals + [[] for _ in range(len(tree.evals) - len(evals))]
    tree.paths = []
    if hasattr(tree, 'rounds'):
        tree.rounds = []
    return len(kept)


def most_visited_root(tree):
    """The move of one root: its legal child with the most visits, ties to the lowest action; -1 without a legal action."""
    acts = tree.legal[0]
    if acts.size == 0:
        return -1
    n = np.array([tree.n[tree.child[0, a]] if tree.child[0, a] >= 0 else 0 for a in acts])
    return int(acts[int(np.argmax(n))])


def search_rounds(trees, rounds, L, evaluator_np, c, komi):
    """`rounds` rounds on the trees as they stand: the loops of pe.expected_puct (L = None) / pl.expected_puct_leaves."""
    R = len(trees)
    for _ in range(rounds):
        if L is None:
            picked = [[(y, -1, b)] for y, b in (t.select(c) for t in trees)]
        else:
            picked = [t.select_round(c, L) for t in trees]
        if R:
            states = np.stack([b for row in picked for _, _, b in row])
            priors, values = evaluator_np(states, mc.legal_mask(states))
            priors, values = np.asarray(priors, np.float32), np.asarray(values, np.float32)
        for r, t in enumerate(trees):
            for j, (y, _, _) in enumerate(picked[r]):
                if y >= 0:
                    row = r * len(picked[r]) + j
                    if L is None:
                        t.backup(y, priors[row], values[row], komi)
                    else:
                        t.backup_slot(y, priors[row], values[row], komi)


def make_trees(roots, capacity, L):
    roots = np.ascontiguousarray(roots, np.uint8)
    return [(pe.Tree if L is None else pl.LeavesTree)(roots[r], capacity - 1) for r in range(roots.shape[0])]


def results(trees, A):
    """The fields of gogame.Puct (pe.ROOT_KEYS, 'tree': pe.TREE_KEYS [R, capacity]) of the trees as they stand."""
    R = len(trees)
    NN = trees[0].n.shape[0] if R else 0
    out = {'legal': np.zeros((R, A), bool), 'visits': np.zeros((R, A), np.int32), 'value_sum': np.zeros((R, A), np.float64),
           'priors': np.zeros((R, A), np.float32)}
    for r, t in enumerate(trees):
        out['legal'][r, t.legal[0]] = True
        has = t.child[0] >= 0
        out['visits'][r, has] = t.n[t.child[0, has]]
        out['value_sum'][r, has] = t.w[t.child[0, has]]
        out['priors'][r] = t.prior[0]
    out['root_visits'] = np.array([t.n[0] for t in trees], np.int32)
    out['root_value_sum'] = np.array([t.w[0] for t in trees], np.float64)
    out['nodes'] = np.array([len(t.boards) for t in trees], np.int32)
    stack = lambda f, dt: np.stack([f(t) for t in trees]).astype(dt) if R else np.zeros((0, NN), dt)
    out['tree'] = {'parent': stack(lambda t: t.parent, np.int32), 'action': stack(lambda t: t.action, np.int32),
                   'visits': stack(lambda t: t.n, np.int32), 'value_sum': stack(lambda t: t.w, np.float64)}
    return out


def next_root(tree, a):
    """The root's board after action a; -1 leaves it."""
    return tree.boards[0] if a == -1 else c_oracle.next_state(tree.boards[0], a)


def expected_puct_play(roots, moves, iterations, evaluator_np, c=1.25, komi=0.0, leaves=None, capacity=None, reuse=True,
                       on_move=None):
    """-> (actions int64 [R, moves], final states uint8 [R, 6, N, N], per move the results() before its advance, the trees):
    gogame.puct_play restated.  on_move(mv, trees, actions, kept), if given, is called after every advance."""
    roots = np.ascontiguousarray(roots, np.uint8)
    R, _, N, _ = roots.shape
    A = N * N + 1
    NN = iterations * (leaves or 1) + 1 if capacity is None else capacity
    trees = make_trees(roots, NN, leaves)
    played = np.zeros((R, moves), np.int64)
    per_move = []
    for mv in range(moves):
        search_rounds(trees, iterations, leaves, evaluator_np, c, komi)
        per_move.append(results(trees, A))
        acts = [most_visited_root(t) for t in trees]
        played[:, mv] = acts
        kept = [advance(t, a, next_root(t, a)) for t, a in zip(trees, acts)]
        if on_move is not None:
            on_move(mv, trees, acts, kept)
        if not reuse:
            trees = make_trees(np.stack([t.boards[0] for t in trees]) if R else roots, NN, leaves)
    final = np.stack([t.boards[0] for t in trees]) if R else roots
    return played, final, per_move, trees
