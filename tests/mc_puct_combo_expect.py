"""Expected results of the PUCT search with its options TOGETHER (gogame.PuctSearch / puct_play / puct_selfplay with leaves=,
capacity=, superko= False / True / 'tree', gumbel= with gumbel_noise=, noise= with eps=, sample_moves=, first_game=, reuse=) -
test infrastructure, CPU only.  Nothing here restates a rule a second time: the three walks (pe.Tree, pl.LeavesTree,
ge.GumbelTree) are composed with the superko rule (se._Rule) by subclassing, the root noise, the visit-count draw and the
read-outs are ps.root_noise / ps.root_policy / GumbelTree.readout, the re-rooting is pa.advance.  What is new is the ORDER in
which a move loop uses them, written from the docstrings of gogame.puct_selfplay / puct_play / PuctSearch:

  1. the state is recorded                     5. noise on the fresh roots round 0 has just evaluated
  2. forbid_root when superko is on            6. the other rounds
  3. noise on kept roots, or set_g             7. root_policy, or the Gumbel read-out
  4. round 0                                   8. advance     9. the new root enters the history

Every run counts what it exercised (`events`), so that a device test can show it did not pass on games where nothing interacted:
root_forbid (a root from which forbid_root took a move), root_forbid_kept_child (.. under which a visited child stood),
deep_marks (nodes below the root that the rule marked when they were made), noise_on_reduced (noise or g drawn for a root whose
legal set the rule has reduced), and GumbelTree's own fallback / past / tie / neg_inf / collision.

Also the inputs of tests/test_gpu_puct_combo.py (the planted roots, the noise and the case tables), whose premises
tests/test_puct_combo_host.py asserts."""
import collections
import functools
import itertools

import numpy as np

import mc_cases as cs
import mc_expect as mc
import mc_gumbel_expect as ge
import mc_puct_advance_expect as pa
import mc_puct_expect as pe
import mc_puct_leaves_expect as pl
import mc_puct_selfplay_expect as ps
import mc_puct_superko_expect as se

MODES = (False, True, 'tree')        # superko= of the move loops: off, the roots only, every node
EVENTS = ('root_forbid', 'root_forbid_kept_child', 'deep_marks', 'noise_on_reduced', 'fallback', 'past', 'tie', 'neg_inf', 'collision')


# ---------------------------------------------------------------- the trees: a walk and the rule
class _Moded:
    """What the three classes share: the rule's state, the mode and the run's event counter."""

    def _init_mode(self, history, mode, tally):
        self._init_rule(history)
        self.mode, self.tally = mode, (collections.Counter() if tally is None else tally)
        self.reduced = False           # the rule has taken an action from node 0 (forbid() and advance() keep it)

    def _made(self, y):
        self.tally['deep_marks'] += bool(self.marks[y])


class Tree(se.SuperkoTree, _Moded):
    def __init__(self, root, I, history, mode, tally=None):
        se.SuperkoTree.__init__(self, root, I, history)
        self._init_mode(history, mode, tally)

    def select(self, c):
        if self.mode != 'tree':
            return pe.Tree.select(self, c)
        y, board = se.SuperkoTree.select(self, c)
        if self.paths[-1][1] >= 0:
            self._made(y)
        return y, board


class LeavesTree(se.SuperkoLeavesTree, _Moded):
    def __init__(self, root, C, history, mode, tally=None):
        se.SuperkoLeavesTree.__init__(self, root, C, history)
        self._init_mode(history, mode, tally)

    def _walk(self, c):
        if self.mode != 'tree':
            return pl.LeavesTree._walk(self, c)
        y, mv, board = se.SuperkoLeavesTree._walk(self, c)
        if mv >= 0:
            self._made(y)
        return y, mv, board


class GumbelTree(ge.GumbelTree, se._Rule, _Moded):
    """ge.GumbelTree with the rule: the walk is GumbelTree's, and a node made now has its pending board replaced by the ruled
    one, exactly as se.SuperkoLeavesTree._walk does; forbid_root is the rule's own; begin, root_terms, choose and readout
    stay GumbelTree's - they read legality from legal[0], which forbid_root reduces."""

    def __init__(self, root, C, schedule, c_visit, c_scale, history, mode, tally=None):
        ge.GumbelTree.__init__(self, root, C, schedule, c_visit, c_scale)
        self._init_mode(history, mode, tally)

    def _walk(self, c):
        y, mv, board = ge.GumbelTree._walk(self, c)
        if self.mode == 'tree' and mv >= 0:
            board = self.pending[y] = self.ruled(y, board)
            self._made(y)
        return y, mv, board


def _keys(roots, histories):
    out = []
    for r in range(len(roots)):
        h = [roots[r]] if histories is None else histories[r]
        out.append([k if isinstance(k, bytes) else se.key_of(k) for k in h])
    return out


def make_trees(roots, histories, capacity, L, mode, tally=None):
    """histories: per root the boards (or position keys) of its game so far, the root included; None = the root alone."""
    roots = np.ascontiguousarray(roots, np.uint8)
    cls = Tree if L is None else LeavesTree
    return [cls(roots[r], capacity - 1, k, mode, tally) for r, k in enumerate(_keys(roots, histories))]


def forbid(tree):
    """PuctSearch.forbid_repeats at one root, counted."""
    before = set(int(a) for a in tree.legal[0])
    tree.forbid_root()
    gone = sorted(before - set(int(a) for a in tree.legal[0]))
    tree.reduced = tree.reduced or bool(gone)
    if gone:
        tree.tally['root_forbid'] += 1
        tree.tally['root_forbid_kept_child'] += any(tree.child[0, a] >= 0 and tree.n[tree.child[0, a]] > 0 for a in gone)


def advance(tree, a):
    """pa.advance and, with the rule on, what the caller's loop does behind it (se.advance): the marks of a root that moved are
    dropped and the new root enters the history.  tree.reduced: the new root's board already carries marks of the rule (a kept
    node of mode 'tree': its invalid plane differs from the one the game's own rules give it)."""
    bare = pa.next_root(tree, a)
    kept = se.advance(tree, a) if tree.mode else pa.advance(tree, a, bare)
    if a != -1:
        tree.reduced = bool((tree.boards[0][3] != bare[3]).any())
    return kept


# ---------------------------------------------------------------- the host side of a Gumbel search with the rule
def gumbel_args(gumbel):
    """gumbel= as an int m or (m, n, c_visit, c_scale) -> the four."""
    if isinstance(gumbel, (int, np.integer)):
        return int(gumbel), None, 50.0, 0.5
    m, n, cv, cs = gumbel
    return int(m), n, float(cv), float(cs)


class GumbelSearch(ge.Search):
    """ge.Search on GumbelTrees with the rule: forbid() is PuctSearch.forbid_repeats, advance() also keeps the histories."""

    def __init__(self, roots, histories, mode, T, L, m, tally=None, **kw):
        roots = np.ascontiguousarray(roots, np.uint8)
        super().__init__(roots, T, L, m, **kw)
        self.mode, self.tally = mode, (collections.Counter() if tally is None else tally)
        self.trees = [GumbelTree(roots[r], old.I, self.schedule, self.c_visit, self.c_scale, k, mode, self.tally)
                      for r, (old, k) in enumerate(zip(self.trees, _keys(roots, histories)))]
        self.begin()

    def forbid(self):
        for t in self.trees:
            forbid(t)

    def advance(self, acts):
        kept = [advance(t, int(a)) for t, a in zip(self.trees, acts)]
        self.begin()
        return kept


def legal_rows(trees, A):
    out = np.zeros((len(trees), A), bool)
    for r, t in enumerate(trees):
        out[r, t.legal[0]] = True
    return out


def harvest(trees, tally):
    """The events the trees counted themselves, added to the run's counter once (when the trees are dropped or the run ends)."""
    for t in trees:
        for k, v in getattr(t, 'events', {}).items():
            tally[k] += v
        tally['collision'] += getattr(t, 'collisions', 0)


class Host:
    """The host side of one gogame.PuctSearch of a move loop, every option together: the plain trees, or a GumbelSearch."""

    def __init__(self, roots, histories, T, evaluator_np, c, komi, leaves, capacity, superko, gumbel, base_of, tally):
        roots = np.ascontiguousarray(roots, np.uint8)
        self.R, self.A = roots.shape[0], roots.shape[-1] ** 2 + 1
        self.T, self.L, self.ev, self.c, self.komi, self.mode, self.tally = T, leaves, evaluator_np, c, komi, superko, tally
        if gumbel is None:
            self.g = None
            NN = T * (leaves or 1) + 1 if capacity is None else capacity
            self.trees = make_trees(roots, histories, NN, leaves, superko, tally)
        else:
            m, n, cv, cs = gumbel_args(gumbel)
            self.g = GumbelSearch(roots, histories, superko, T, leaves, m, tally=tally, n=n, c=c, komi=komi, c_visit=cv, c_scale=cs,
                                  capacity=capacity, base_of=base_of)
            self.trees = self.g.trees

    def boards(self):
        return np.stack([t.boards[0] for t in self.trees])

    def legal(self):
        return legal_rows(self.trees, self.A)

    def forbid(self):
        for t in self.trees:
            forbid(t)

    def reduced(self):
        return sum(bool(t.reduced) for t in self.trees)

    def rounds(self, k):
        if self.g is None:
            pa.search_rounds(self.trees, k, self.L, self.ev, self.c, self.komi)
        else:
            for _ in range(k):
                self.g.round(self.ev)

    def advance(self, acts):
        if self.g is not None:
            return self.g.advance(acts)
        return [advance(t, int(a)) for t, a in zip(self.trees, acts)]


def _records(R, moves, A, N):
    return {'actions': np.full((R, moves), -1, np.int64), 'pi': np.zeros((R, moves, A), np.float32),
            'value': np.zeros((R, moves), np.float32), 'lengths': np.zeros(R, np.int32),
            'states': np.zeros((R, moves, 6, N, N), np.uint8)}


def expected_selfplay(roots, moves, iterations, evaluator_np, c=1.25, komi=0.0, leaves=None, capacity=None, superko=False,
                      gumbel=None, g_of=None, noise=None, eps=0.25, sample_moves=0, seed=20260927, first_game=0,
                      base_of=ge.numpy_base, histories=None):
    """gogame.puct_selfplay(.., record_states=True) restated with every option together -> dict of the SelfPlay fields plus
    'trees', 'rng', 'events' (a Counter over EVENTS) and 'host'.  gumbel: None, m or (m, n, c_visit, c_scale); g_of(mv, legal) /
    noise(mv, legal) -> float32 [R, A] or None; base_of: as ge.Search.  histories: what the games' PositionHistory holds
    beside the roots (None: the roots alone, as puct_selfplay seeds it)."""
    roots = np.ascontiguousarray(roots, np.uint8)
    R, _, N, _ = roots.shape
    A = N * N + 1
    assert superko in MODES and (gumbel is None or (noise is None and sample_moves == 0)) and (gumbel is not None or g_of is None)
    tally = collections.Counter()
    host = Host(roots, histories, iterations, evaluator_np, c, komi, leaves, capacity, superko, gumbel, base_of, tally)
    rng = ps.seeds(R, seed, first_game)
    out = _records(R, moves, A, N)
    for mv in range(moves):
        out['states'][:, mv] = host.boards()                                   # 1. (before forbid_repeats marks the root)
        if superko:
            host.forbid()                                                      # 2.
        if noise is not None:                                                  # 3. the roots kept from the move before
            z = np.asarray(noise(mv, host.legal()), np.float32)
            tally['noise_on_reduced'] += host.reduced()
            todo = [ps.root_noise(t, z[r], eps, 1) for r, t in enumerate(host.trees)]
        if g_of is not None:
            host.g.set_g(g_of(mv, host.legal()))
            tally['noise_on_reduced'] += host.reduced()
        host.rounds(1)                                                         # 4.
        if noise is not None:                                                  # 5.
            todo = [ps.root_noise(t, z[r], eps, todo[r]) for r, t in enumerate(host.trees)]
        host.rounds(iterations - 1)                                            # 6.
        if host.g is None:                                                     # 7.
            for r, t in enumerate(host.trees):
                out['actions'][r, mv], out['pi'][r, mv], out['value'][r, mv], rng[r] = ps.root_policy(t, mv < sample_moves, rng[r])
        else:
            acts, _, _, val, pi = host.g.readout()
            out['actions'][:, mv], out['pi'][:, mv], out['value'][:, mv] = acts, pi, val
        out['lengths'] += out['actions'][:, mv] >= 0
        host.advance(out['actions'][:, mv])                                    # 8., 9.
    harvest(host.trees, tally)
    out['final_states'] = host.boards()
    out['outcome'] = np.array([ps.outcome(t.boards[0], komi) for t in host.trees], np.int8)
    out['trees'], out['rng'], out['events'], out['host'] = host.trees, rng, tally, host
    return out


def expected_play(roots, moves, iterations, evaluator_np, c=1.25, komi=0.0, leaves=None, capacity=None, superko=False, gumbel=None,
                  g_of=None, reuse=True, base_of=ge.numpy_base, histories=None):
    """gogame.puct_play restated with every option together -> (actions int64 [R, moves], final states, the last Host, events).
    reuse=False: after every move a new search on the next boards (the move played on node 0's board alone), with the whole
    history."""
    roots = np.ascontiguousarray(roots, np.uint8)
    R = roots.shape[0]
    assert superko in MODES and (gumbel is not None or g_of is None)
    tally = collections.Counter()
    make = lambda boards, hist: Host(boards, hist, iterations, evaluator_np, c, komi, leaves, capacity, superko, gumbel, base_of, tally)
    host = make(roots, histories)
    played = np.zeros((R, moves), np.int64)
    for mv in range(moves):
        if superko:
            host.forbid()
        if g_of is not None:
            host.g.set_g(g_of(mv, host.legal()))
            tally['noise_on_reduced'] += host.reduced()
        host.rounds(iterations)
        acts = [pa.most_visited_root(t) for t in host.trees] if host.g is None else host.g.readout()[0]
        played[:, mv] = acts
        if reuse:
            host.advance(acts)
        else:
            nxt = np.stack([pa.next_root(t, int(a)) for t, a in zip(host.trees, acts)])
            hist = [sorted(t.history | {se.key_of(b)}) for t, b in zip(host.trees, nxt)] if superko else None
            harvest(host.trees, tally)
            host = make(nxt, hist)
    harvest(host.trees, tally)
    return played, host.boards(), host, tally


# ---------------------------------------------------------------- noise that depends on the legal set it is given
def _count(legal):
    return mc.to_np(legal).astype(np.int64).sum(axis=1)[:, None]


def dyadic_g(rows, salt=0):
    """g_of(mv, legal) for the global rows `rows`: draws exact in float32 (multiples of 1 / 64 in [-2, 6)), a function of (row,
    action, move, the NUMBER of legal actions of the row): a search that hands over another legal set gets other draws."""
    rows = np.asarray(rows, np.int64)[:, None]

    def g_of(mv, legal):
        a = np.arange(mc.to_np(legal).shape[1], dtype=np.int64)[None, :]
        k = ((rows * 7919 + a * 104729 + (mv + 1) * 1299709 + salt * 15485863 + _count(legal) * 32452843) * 2654435761 >> 11) % 512
        return (k.astype(np.float32) - np.float32(128)) / np.float32(64)

    return g_of


def odd_noise(rows, salt=0):
    """noise(mv, legal) for the global rows `rows`: float32 in (0, 1] with NaN, negatives, -0 and +inf strewn in, nothing masked
    by legality, a function of (row, action, move, the number of legal actions of the row)."""
    rows = np.asarray(rows, np.int64)[:, None]

    def noise(mv, legal):
        A = mc.to_np(legal).shape[1]
        k = ((rows * A + np.arange(A, dtype=np.int64)[None, :]) * 37 + (mv + salt) * 101 + _count(legal) * 53) % 64
        z = ((k + 1).astype(np.float32) / np.float32(64)).astype(np.float32)
        for m, v in ((3, np.nan), (5, -1.0), (7, -0.0), (11, np.inf)):
            z = np.where(k % 16 == m, np.float32(v), z).astype(np.float32)
        return z

    return noise


# ---------------------------------------------------------------- the move loops' cases: a pairwise covering set
FACTORS = (('leaves', (None, 1, 3)), ('gumbel', (None, 4)), ('superko', MODES), ('noise', (False, True)), ('sample_moves', (0, 2)),
           ('gumbel_noise', (False, True)), ('reuse', (True, False)), ('capacity', ('default', 'room')))


def allowed(case):
    """What the two loops accept: puct_selfplay always reuses; noise and sample_moves are its own and only without gumbel;
    gumbel_noise only with gumbel."""
    if case['fn'] == 'selfplay':
        if not case['reuse']:
            return False
    elif case['noise'] or case['sample_moves']:
        return False
    if case['gumbel'] is None:
        return not case['gumbel_noise']
    return not case['noise'] and not case['sample_moves']


def every_case():
    keys = [k for k, _ in FACTORS]
    for fn in ('selfplay', 'play'):
        for values in itertools.product(*[v for _, v in FACTORS]):
            case = dict(zip(keys, values), fn=fn)
            if allowed(case):
                yield case


def pairs_of(case):
    items = [(k, case[k]) for k, _ in FACTORS]
    return {frozenset(p) for p in itertools.combinations(items, 2)}


def allowed_pairs():
    """Every pair of option values that some call of puct_selfplay or puct_play can carry."""
    out = set()
    for case in every_case():
        out |= pairs_of(case)
    return out


@functools.lru_cache(maxsize=None)
def _covering():
    todo, picked, cases = allowed_pairs(), [], list(every_case())
    while todo:
        best = max(cases, key=lambda c: len(pairs_of(c) & todo))      # (max keeps the first of equals: a fixed order)
        picked.append(best)
        todo -= pairs_of(best)
    return tuple(tuple(sorted(c.items(), key=lambda kv: kv[0])) for c in picked)


def covering_cases():
    """The cases of the move-loop test, greedily chosen: every allowed pair of option values occurs in one of them."""
    return [dict(c) for c in _covering()]


def case_id(case):
    return '-'.join(str(case[k]) for k in ('fn',) + tuple(k for k, _ in FACTORS))


EXTRA_CASES = tuple(dict(fn='selfplay', leaves=3, gumbel=4, superko=mode, noise=False, sample_moves=0, gumbel_noise=True, reuse=True,
                         capacity='room') for mode in (True, 'tree'))       # what a trainer runs: Gumbel self-play under the rule


def loop_cases():
    return covering_cases() + [dict(c) for c in EXTRA_CASES]


def needs(case):
    """The event a case must show (the issue's conditions) or None."""
    if case['superko'] == 'tree':
        return 'deep_marks'
    return 'root_forbid_kept_child' if case['superko'] is True and case['reuse'] else None


LOOP = {2: dict(moves=12, T=4, name='hash'), 5: dict(moves=12, T=6, name='hostile')}      # per board size: moves and rounds per move of the move-loop cases
LOOP_KW = dict(c=1.25, komi=0.5, seed=7, first_game=4)


def run_loop_case(case, roots, ids, N, evaluator_np, base_of=ge.numpy_base):
    """One case of the move-loop test on the restatement -> expected_selfplay's dict, or expected_play's tuple.  ids: the
    identity of every root (what its noise depends on)."""
    moves, T = LOOP[N]['moves'], LOOP[N]['T']
    L = case['leaves']
    kw = dict(c=LOOP_KW['c'], komi=LOOP_KW['komi'], leaves=L, superko=case['superko'], gumbel=case['gumbel'], base_of=base_of,
              capacity=moves * T * (L or 1) + 1 if case['capacity'] == 'room' else None,
              g_of=dyadic_g(ids, salt=5) if case['gumbel_noise'] else None)
    if case['fn'] == 'play':
        return expected_play(roots, moves, T, evaluator_np, reuse=case['reuse'], **kw)
    return expected_selfplay(roots, moves, T, evaluator_np, noise=odd_noise(ids, salt=3) if case['noise'] else None, eps=0.25,
                             sample_moves=case['sample_moves'], seed=LOOP_KW['seed'], first_game=LOOP_KW['first_game'], **kw)


# ---------------------------------------------------------------- the roots of the move loops
# puct_selfplay and puct_play seed their PositionHistory with the roots alone, so at N = 5 the rule has to fire from the games
# themselves.  Random play does that seldom beyond 3x3 (mid-game roots of mc_cases.stack(5): no root event in 16 moves), so the
# roots are late positions - a handful of legal points, stones in atari, captures that give stones back - picked from
# mc_cases.late_roots(5, seed)[i] by a scan over 600 of them for the ones whose games run into the rule: (seed, i).
LATE5 = ((27, 3), (32, 2), (50, 5), (53, 2), (37, 4), (61, 1), (28, 2), (35, 4), (8, 3), (4, 1), (20, 0), (23, 4))


@functools.lru_cache(maxsize=None)
def loop_roots(N):
    """-> (roots uint8 [R, 6, N, N], ids): N = 2: the size's roots; N = 5: the planted late roots, a finished game and the empty
    board."""
    if N == 2:
        roots = cs.stack(2)
        return roots, tuple(range(len(roots)))
    assert N == 5
    late = [cs.late_roots(5, seed=s, count=6)[i] for s, i in LATE5]
    roots = np.stack(late + [cs.size_roots(5)['ended'], cs.size_roots(5)['empty']])
    roots.setflags(write=False)
    return roots, tuple(s * 6 + i for s, i in LATE5) + (1, 2)


# ---------------------------------------------------------------- planted histories for searches driven step by step
def plant(roots, T, L, gumbel, evaluator_np, g_of=None, **kw):
    """Per root a game record that makes the rule fire on move 0 or 1 of a search driven by hand on its own PositionHistory ->
    histories (per root the boards of its record, the root last).  The same search WITHOUT the rule runs one move; below the
    child under the move it plays, the most visited grandchild under a board move (ties to the lowest action) is the planted
    position P2, recorded as if the game had been there.  The ruled search is the same search until the rule acts: with
    superko='tree' the node under the move is marked when it is made (a deep mark in move 0), with True it becomes the root of
    move 1 with a visited child under a move forbid_root now takes away.  A root without such a grandchild keeps the record of
    itself alone."""
    roots = np.ascontiguousarray(roots, np.uint8)
    N = roots.shape[-1]
    host = Host(roots, None, T, evaluator_np, kw.get('c', 1.25), kw.get('komi', 0.0), L, kw.get('capacity'), False, gumbel,
                ge.numpy_base, collections.Counter())
    if g_of is not None:
        host.g.set_g(g_of(0, host.legal()))
    host.rounds(T)
    acts = [pa.most_visited_root(t) for t in host.trees] if host.g is None else host.g.readout()[0]
    out = []
    for r, (t, a) in enumerate(zip(host.trees, acts)):
        y = int(t.child[0, a]) if a >= 0 else -1
        best = None
        if y >= 0 and t.boards[y] is not None:
            for b in t.legal[y]:
                k = int(t.child[y, b])
                if b < N * N and k >= 0 and t.boards[k] is not None and t.n[k] > 0 and (best is None or t.n[k] > t.n[best]):
                    best = k
        out.append([roots[r]] if best is None else [t.boards[best], roots[r]])
    return out


def _step(N, mode, name, T, L, m, moves, names=None):
    return dict(N=N, mode=mode, name=name, T=T, L=L, m=m, moves=moves, names=names)


PLANTED_NAMES = ('late0', 'late1', 'late2', 'mid0', 'mid1', 'ended')
STEP_CASES = ([_step(2, mode, name, T, L, m, 16) for mode in (True, 'tree') for name in ('hostile', 'hash')
               for T, L, m in ((4, 2, 4), (6, 3, 2), (8, 1, 4))]
              + [_step(N, mode, ('hostile', 'hash')[(N + (mode is True)) % 2], 4, 2, 2, 3, PLANTED_NAMES) for N in (3, 9, 19)
                 for mode in (True, 'tree')]
              + [_step(2, 'tree', 'hash', 8, None, 4, 16), _step(9, True, 'hash', 8, None, 2, 3, PLANTED_NAMES)])
STEP_KW = dict(c=1.25, komi=0.5)
STAY = (1, 1)            # (move, root): this root does not move in that move (action -1)


def step_id(case):
    return '-'.join(str(case[k]) for k in ('N', 'mode', 'name', 'T', 'L', 'm'))


@functools.lru_cache(maxsize=None)
def _step_inputs(key):
    case = dict(key)
    N, T, L = case['N'], case['T'], case['L']
    roots = cs.stack(N, case['names'])
    g_of = dyadic_g(range(len(roots)), salt=N)
    capacity = case['moves'] * T * (L or 1) + 1
    hist = None
    if case['names'] is not None:
        hist = plant(roots, T, L, case['m'], ge.EVALUATORS[case['name']][0], g_of, capacity=capacity, **STEP_KW)
    return roots, hist, g_of, capacity


def step_inputs(case):
    """-> (roots, histories or None, g_of, capacity) of a step-by-step case; planted where the case names its roots."""
    return _step_inputs(tuple(sorted(case.items(), key=lambda kv: kv[0])))


def step_search(case, base_of=ge.numpy_base):
    roots, hist, _, capacity = step_inputs(case)
    return GumbelSearch(roots, hist, case['mode'], case['T'], case['L'], case['m'], capacity=capacity, base_of=base_of, **STEP_KW)


def run_steps(case):
    """The step-by-step case on the restatement alone -> the GumbelSearch afterwards (its tally holds every event)."""
    s = step_search(case)
    _, _, g_of, _ = step_inputs(case)
    ev = ge.EVALUATORS[case['name']][0]
    for mv in range(case['moves']):
        s.forbid()
        s.set_g(g_of(mv, legal_rows(s.trees, s.A)))
        s.tally['noise_on_reduced'] += sum(bool(t.reduced) for t in s.trees)
        for _ in range(case['T']):
            s.round(ev)
        acts = s.readout()[0].copy()
        if mv == STAY[0]:
            assert acts[STAY[1]] >= 0
            acts[STAY[1]] = -1
        s.advance(acts)
    harvest(s.trees, s.tally)
    return s


# ---------------------------------------------------------------- the plane cases (every hand-out option on, superko='tree')
PLANE_T, PLANE_L, PLANE_MOVES, PLANE_SYM = 4, 2, 3, 4711
PLANE_NAMES = PLANTED_NAMES[:5] + ('ko', 'ended')
PLANE_CASES = tuple((N, gumbel) for N in (5, 9) for gumbel in (None, 4))


@functools.lru_cache(maxsize=None)
def plane_inputs(N, gumbel):
    """-> (roots, planted histories, g_of or None, capacity) of a plane case: the hash evaluator, three moves."""
    roots = cs.stack(N, PLANE_NAMES)
    g_of = dyadic_g(range(len(roots)), salt=40 + N) if gumbel is not None else None
    capacity = PLANE_MOVES * PLANE_T * PLANE_L + 1
    hist = plant(roots, PLANE_T, PLANE_L, gumbel, pe.hash_evaluator_np, g_of, capacity=capacity, **STEP_KW)
    return roots, hist, g_of, capacity


def plane_host(N, gumbel, base_of=ge.numpy_base):
    roots, hist, _, capacity = plane_inputs(N, gumbel)
    return Host(roots, hist, PLANE_T, pe.hash_evaluator_np, STEP_KW['c'], STEP_KW['komi'], PLANE_L, capacity, 'tree', gumbel, base_of,
                collections.Counter())


def plane_move(host, mv, g_of):
    """One move of a plane case on the restatement -> the actions played (most visits, or the Gumbel action)."""
    host.forbid()
    if g_of is not None:
        host.g.set_g(g_of(mv, host.legal()))
    host.rounds(PLANE_T)
    acts = np.array([pa.most_visited_root(t) for t in host.trees], np.int64) if host.g is None else host.g.readout()[0].astype(np.int64)
    host.advance(acts)
    return acts


# ---------------------------------------------------------------- the shard cases (puct_selfplay of the plane configuration)
SHARD_MOVES, SHARD_T, SHARD_L, SHARD_SEED, SHARD_FIRST = 8, 4, 2, 11, 1
LATE9 = ((22, 3), (87, 5), (99, 3), (26, 4), (81, 5), (36, 0), (61, 1), (37, 1), (72, 5), (7, 0))     # as LATE5, from a scan of 650
SHARD_CASES = tuple((N, gumbel) for N in (5, 9) for gumbel in (None, 4))


@functools.lru_cache(maxsize=None)
def shard_roots(N):
    """-> (roots, ids, cut): cut is odd - no multiple of the two leaves a root hands out."""
    if N == 5:
        roots, ids = loop_roots(5)
        return roots, ids, 5
    late = [cs.late_roots(9, seed=s, count=6)[i] for s, i in LATE9]
    roots = np.stack(late + [cs.size_roots(9)['ended'], cs.size_roots(9)['mid0']])
    roots.setflags(write=False)
    return roots, tuple(s * 6 + i for s, i in LATE9) + (1, 2), 5


def shard_kw(gumbel, ids):
    """The options of a shard case that the restatement knows (the planes, symmetry= and past= leave the records alone)."""
    kw = dict(c=STEP_KW['c'], komi=STEP_KW['komi'], leaves=SHARD_L, capacity=SHARD_MOVES * SHARD_T * SHARD_L + 1, seed=SHARD_SEED)
    if gumbel is None:
        return dict(kw, noise=odd_noise(ids, salt=6), eps=0.25, sample_moves=2)
    return dict(kw, gumbel=gumbel, **{'g_of': dyadic_g(ids, salt=8)})


def expected_shard(N, gumbel, point_evaluator, rows=slice(None), first_game=SHARD_FIRST, base_of=ge.numpy_base):
    """puct_selfplay of a shard case on the restatement: the evaluator of planes wrapped in the orientations the search draws."""
    import features_expect as fe
    import symmetry_expect as sy
    roots, ids, _ = shard_roots(N)
    W = sy.wrapped(point_evaluator, PLANE_SYM + N, first_row=first_game * SHARD_L)
    return expected_selfplay(roots[rows], SHARD_MOVES, SHARD_T, lambda states, legal: W(fe.batch_features(states), legal),
                             superko='tree', first_game=first_game, base_of=base_of, **shard_kw(gumbel, ids[rows]))
