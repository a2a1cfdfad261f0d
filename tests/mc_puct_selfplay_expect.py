"""Expected results of PUCT self-play (gogame.PuctSearch.add_root_noise / root_policy, gogame.puct_selfplay:
gg_puct_root_noise / gg_puct_root_policy) - test infrastructure, CPU only.  Builds on tests/mc_puct_advance_expect.py:
root_noise() and root_policy() work on a Tree / LeavesTree outside a round and are written from the text of
include/gymgo_amd.h - the float32 operations through np.float32 in the stated order, the generator's ply step in Python
integers -; expected_selfplay() is the move loop of gogame.puct_selfplay."""
import numpy as np

import mc_expect as mc
import mc_puct_expect as pe
import mc_puct_advance_expect as pa

MASK64 = 2 ** 64 - 1
QUIET_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def splitmix_step(x):
    """One ply step of the generator: -> (the new state, its 64-bit output)."""
    x = (int(x) + mc.GOLDEN_GAMMA) & MASK64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return x, z ^ (z >> 31)


def seeds(R, seed, first_game=0):
    """The generators of gogame.rng_seed(R, seed, first_game) as Python integers."""
    return [int(v) for v in mc.po_seed(seed, first_game + np.arange(R, dtype=np.int64))]


def mix(keep, p, eps, z):
    """(keep * p) + (eps * z) in float32, three roundings; z with NaN, negatives and -0 as +0; a NaN result is the quiet NaN."""
    z = np.float32(z)
    z = z if z > 0 else np.float32(0)
    with np.errstate(all='ignore'):
        a = np.float32(keep) * np.float32(p)
        b = np.float32(eps) * z
        s = np.float32(a + b)
    return QUIET_NAN if s != s else s


def root_noise(tree, noise, eps, todo):
    """gg_puct_root_noise on one root -> the new todo (0 / 1).  noise: float32 [A]."""
    assert not getattr(tree, 'pending', None) and not getattr(tree, 'v', np.zeros(1)).any()
    if not todo or tree.n[0] <= 0 or tree.legal[0].size == 0:
        return int(todo)
    keep = np.float32(1) - np.float32(eps)
    row = np.zeros(tree.prior.shape[1], np.float32)
    for a in tree.legal[0]:
        row[a] = mix(keep, tree.prior[0, a], np.float32(eps), np.asarray(noise, np.float32)[a])
    tree.prior[0] = row
    return 0


def root_visits(tree):
    """int64 [A]: n of the child under every legal action of the root, 0 elsewhere."""
    n = np.zeros(tree.prior.shape[1], np.int64)
    for a in tree.legal[0]:
        k = int(tree.child[0, a])
        n[a] = int(tree.n[k]) if k >= 0 else 0
    return n


def root_policy(tree, sample, rng):
    """gg_puct_root_policy on one root -> (action, pi float32 [A], value float32, the generator afterwards)."""
    assert not getattr(tree, 'pending', None) and not getattr(tree, 'v', np.zeros(1)).any()
    A = tree.prior.shape[1]
    pi = np.zeros(A, np.float32)
    if tree.legal[0].size == 0:
        return -1, pi, np.float32(0), int(rng)
    n = root_visits(tree)
    S = int(n.sum())
    assert S < 2 ** 31
    if S > 0:
        for a in tree.legal[0]:
            pi[a] = np.float32(int(n[a])) / np.float32(S)
    s = -1.0 if tree.boards[0][2, 0, 0] != 0 else 1.0
    value = np.float32(s * float(tree.w[0]) / float(tree.n[0])) if tree.n[0] > 0 else np.float32(0)
    if not sample or S == 0:
        return pa.most_visited_root(tree), pi, value, int(rng)
    x, u = splitmix_step(rng)
    k = ((u >> 32) * S) >> 32
    run = 0
    for a in tree.legal[0]:                       # ascending
        run += int(n[a])
        if run > k:
            return int(a), pi, value, x
    raise AssertionError('k < S: some running sum exceeds it')


def outcome(board, komi):
    """int: sign(black area - white area - komi) by the search's terminal rule for a game that ended, 0 for a running one."""
    return int(pe.terminal_value(board, komi)) if board[5, 0, 0] != 0 else 0


def expected_selfplay(roots, moves, iterations, evaluator_np, c=1.25, komi=0.0, leaves=None, capacity=None, noise=None,
                      eps=0.25, sample_moves=0, seed=20260927, first_game=0):
    """-> dict of the fields of gogame.SelfPlay (NumPy; 'states' always recorded) plus 'trees' and 'rng' (the generators
    afterwards, Python integers): gogame.puct_selfplay restated.  noise: None or noise(mv, legal bool [R, A]) -> float32
    [R, A]."""
    roots = np.ascontiguousarray(roots, np.uint8)
    R, _, N, _ = roots.shape
    A = N * N + 1
    NN = iterations * (leaves or 1) + 1 if capacity is None else capacity
    trees = pa.make_trees(roots, NN, leaves)
    rng = seeds(R, seed, first_game)
    out = {'actions': np.full((R, moves), -1, np.int64), 'pi': np.zeros((R, moves, A), np.float32),
           'value': np.zeros((R, moves), np.float32), 'lengths': np.zeros(R, np.int32),
           'states': np.zeros((R, moves, 6, N, N), np.uint8)}
    for mv in range(moves):
        if R:
            out['states'][:, mv] = np.stack([t.boards[0] for t in trees])
        if noise is not None:
            legal = np.zeros((R, A), bool)
            for r, t in enumerate(trees):
                legal[r, t.legal[0]] = True
            z = np.asarray(noise(mv, legal), np.float32)
            todo = [root_noise(t, z[r], eps, 1) for r, t in enumerate(trees)]
        pa.search_rounds(trees, 1, leaves, evaluator_np, c, komi)
        if noise is not None:
            todo = [root_noise(t, z[r], eps, todo[r]) for r, t in enumerate(trees)]
        pa.search_rounds(trees, iterations - 1, leaves, evaluator_np, c, komi)
        for r, t in enumerate(trees):
            a, out['pi'][r, mv], out['value'][r, mv], rng[r] = root_policy(t, mv < sample_moves, rng[r])
            out['actions'][r, mv] = a
            out['lengths'][r] += a >= 0
            pa.advance(t, a, pa.next_root(t, a))
    out['final_states'] = np.stack([t.boards[0] for t in trees]) if R else roots
    out['outcome'] = np.array([outcome(t.boards[0], komi) for t in trees], np.int8)
    out['trees'], out['rng'] = trees, rng
    return out
