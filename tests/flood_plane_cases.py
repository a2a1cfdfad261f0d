"""The flood-deep boards of tests/flood_cases.py as input of the PLANE kernels and the playout policies, at EVERY board size from 2
to 19, and what is expected of them - test infrastructure, CPU only, NumPy, the C oracle (for plane 3 only) and the definitional
expect modules only; no reference of its own.  tests/test_flood_planes_host.py asserts the premises, tests/test_gpu_flood_planes.py
sends the boards through every plane kernel and through the three playout policies.

boards(N): the first ceil(4 K / 3) boards of flood_cases.batch(N), K the number of crafted boards - every crafted board, and every
fourth board a random position - in two forms:
  forced   as crafted: plane 3 of a capture / atari / join board is 1 everywhere but at q.  A kernel has to take plane 3 as given.
  genuine  plane 3 of those boards from the oracle: q, the snake's other liberties and the empty corners are real candidates.
The two forms differ on the boards of the forced kinds only, and only in plane 3.  An expectation is computed once per process for
the genuine form; the forced form recomputes the rows of the forced kinds and shares the others.  A family that does not read
plane 3 (group liberties, life, area, status, the position hash, the eye mask) has ONE expectation for both forms.

LADDER_ALL_UP_TO: the ladder reader of tests/ladder_expect.py takes about 5 s per 24 boards at 19x19, and the oriented call has
to be searched again (turned first, then searched).  Up to this size the ladder runs on every board; above it on ladder_subset(N):
of every turned kind the unturned and the quarter-turned variant with either colour to move, and two shape boards and two random
positions per colour to move."""
import functools
from types import SimpleNamespace

import numpy as np

import area_expect as ae
import features_expect as fe
import flood_cases as fc
import hash_expect as he
import ladder_expect as lad
import life_expect as life
import mc_expect as mc
import mc_pattern_expect as mq
import mc_policy_expect as mp
import mc_prior_expect as mpr
import mc_tactics_expect as mt
import outcome_expect as oe
import status_expect as se

SIZES = fc.SIZES
FORMS = ('forced', 'genuine')
FAMILIES = ('features', 'life', 'ladder', 'outcome', 'hash', 'area', 'status', 'tactics', 'patterns', 'priors', 'eyes')
READS_PLANE_3 = ('features', 'ladder', 'outcome', 'hash', 'tactics', 'patterns', 'priors')      # (hash: the move hashes)
LADDER_ALL_UP_TO = 12
PRIORS = (('default', mpr.DEFAULT), ('lopsided', mpr.LOPSIDED))
POLICIES = ('no_eye_fill', 'tactical', 'pattern')
ROLLOUT_CELLS = tuple(fc.POLICY_CELLS) + ((24, 1),)
PLAYOUTS, PLAYOUT_PLIES, PLAYOUT_SLOTS = 4, 12, (24, 200)


def _frozen(c):
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, SimpleNamespace):
            _frozen(v)
    return c


@functools.lru_cache(maxsize=None)
def boards(N):
    """-> .forced, .genuine uint8 [B, 6, N, N]; .kind (B names, 'random' among them), .index int32 [B] (into flood_cases.cases(N),
    -1 on random boards), .variant int32 [B] (orientation + 8 x white to move; the index on shape boards; -1 on random boards),
    .q int32 [B] (the forced action, -1 where none), .point int32 [B] (the point the board is about, -1 where none), .seed int32
    [B, 2], .differs (the rows on which the forms differ).  Read only."""
    from oracle import c_oracle
    c, b = fc.cases(N), fc.batch(N)
    K = len(c.kind)
    B = -(-4 * K // 3)
    forced = b.states[:B].copy()
    index = b.index[:B].copy()
    assert set(index[index >= 0].tolist()) == set(range(K))
    kind = list(b.kind[:B])
    genuine = forced.copy()
    differs = np.array([i for i in range(B) if kind[i] in fc.FORCED], np.int64)
    for i in differs:
        genuine[i, 3] = c_oracle.compute_invalid_moves(forced[i], 1 - int(forced[i, 2, 0, 0]), -1)
    pick = lambda a, none: np.where(index >= 0, a[np.maximum(index, 0)].T, none).T.astype(np.int32)
    return _frozen(SimpleNamespace(N=N, forced=forced, genuine=genuine, kind=kind, index=index, variant=pick(c.variant, -1),
                                   q=b.q[:B].copy(), point=pick(c.point, -1), seed=pick(c.seed, -1), differs=differs))


def states_of(N, form):
    return getattr(boards(N), form)


def ladder_subset(N):
    """the rows of boards(N) the ladder is checked on (see the module's docstring): all of them up to LADDER_ALL_UP_TO"""
    b = boards(N)
    B = len(b.kind)
    if N <= LADDER_ALL_UP_TO:
        return np.arange(B)
    rows, seen = [], {}
    for i in range(B):
        white = int(b.forced[i, 2, 0, 0])
        if b.kind[i] in fc.TURNED:
            key = (b.kind[i], int(b.variant[i]))
            take = (b.variant[i] & 7) in (0, 1) and key not in seen
        else:
            key = (b.kind[i], white, sum(1 for k in seen if k[:2] == (b.kind[i], white)))
            take = key[2] < 2
        if take:
            seen[key] = i
            rows.append(i)
    return np.array(rows, np.int64)


def mixed(n):
    """the views of tests/test_gpu_life.mixed: all eight orientations in every wave, with negative and large words"""
    import test_gpu_life
    return test_gpu_life.mixed(n)


def last_variants(N, B):
    """the `last=` forms of the pattern planes and the priors: none, and mc_pattern_expect.last_cycle's"""
    return (('none', None), ('cycle', mq.last_cycle(N, B)))


# ---------------------------------------------------------------- the expectations, family by family
def _features(s):
    return SimpleNamespace(planes=fe.batch_features(s))


def _libs(s):
    return SimpleNamespace(libs=fe.batch_group_liberties(s))


def _life(s):
    planes = life.batch_life(s)
    return SimpleNamespace(planes=planes, settled=life.settled_of(planes))


def _ladder(s):
    planes, aborted = lad.batch_ladder(s)
    return SimpleNamespace(planes=planes, aborted=aborted)


def _outcome(s):
    raw = oe.batch_outcome(s)
    return SimpleNamespace(raw=raw, counts=oe.counts_of(raw), planes=oe.planes_of(raw))


def _move_hashes(s):
    return SimpleNamespace(moves=he.batch_move_hashes(s))


def _hashes(s):
    return SimpleNamespace(hashes=he.batch_hash(s))


def _area(s):
    c = SimpleNamespace(planes=ae.batch_area_planes(s), black=ae.batch_area_planes(s, 0), white=ae.batch_area_planes(s, 1))
    c.counts, c.counts_black, c.counts_white = ae.counts(c.planes), ae.counts(c.black), ae.counts(c.white)
    return c


def _tactics(s):
    return SimpleNamespace(planes=np.stack(mt.tiers(s), axis=1).astype(np.uint8))


def _eyes(s):
    return SimpleNamespace(mask=mp.eyes(s).astype(np.uint8))


def _per_board(fn, N, form, rows=None, turn=False):
    return _per_board_once(fn, N, form, rows, turn)       # (one cache entry whichever way the defaults are spelt)


@functools.lru_cache(maxsize=None)
def _per_board_once(fn, N, form, rows, turn):
    """fn of the boards of one form - all of them, or the tuple `rows`; turn: in the views mixed(their number) -, computed once,
    read only: the genuine form whole, the forced form from it with the rows of the forced kinds computed again."""
    import symmetry_expect as sym
    b = boards(N)
    idx = np.arange(len(b.kind)) if rows is None else np.array(rows, np.int64)
    orient = mixed(len(idx)) & 7
    of = lambda s, i: fn(np.ascontiguousarray(sym.orient_images(s[idx[i]], orient[i])) if turn else s[idx[i]])
    if form == 'genuine':
        return _frozen(of(b.genuine, np.arange(len(idx))))
    out = SimpleNamespace(**{k: np.array(v, copy=True) for k, v in vars(_per_board(fn, N, 'genuine', rows, turn)).items()})
    redo = np.flatnonzero(np.isin(idx, b.differs))
    if len(redo):
        again = of(b.forced, redo)
        for k, v in vars(out).items():
            v[redo] = getattr(again, k)
    return _frozen(out)


def _merge(*parts):
    out = SimpleNamespace()
    for p in parts:
        vars(out).update(vars(p))
    return out


@functools.lru_cache(maxsize=None)
def status_of(N, threshold):
    """generated ownership counts (status_expect.generated: chains on and one count below either inequality) on the boards of N and
    the planes and counts from both sides; the same for both forms"""
    s = boards(N).genuine
    num, den = threshold
    K = se.PLAYOUTS[threshold]
    own, info = se.generated(s, K, num, den, seed=N)
    c = SimpleNamespace(own=own, K=K, num=num, den=den, info=info)
    c.black, c.counts_black = se.batch_status(s, own, K, num, den, side=0)
    c.white, c.counts_white = se.white_view(c.black, c.counts_black)
    white = s[:, 2, 0, 0] != 0
    c.planes = np.where(white[:, None, None, None], c.white, c.black)
    c.counts = np.where(white[:, None], c.counts_white, c.counts_black)
    return _frozen(c)


@functools.lru_cache(maxsize=None)
def expectation(N, form, family):
    """One of FAMILIES on boards(N) in one of FORMS, computed once per process, read only:
    features  .planes [B, 16, N, N], .libs [B, N, N]           life      .planes [B, 4, N, N], .settled [B]
    ladder    .rows (ladder_subset(N)), .planes [n, 4, N, N], .aborted [n]; the oriented call: oriented_ladder(N, form)
    outcome   .raw [B, 4, N, N], .counts [B, 3, N, N], .planes [B, 12, N, N]
    hash      .hashes [B], .moves [B, N*N + 1]                  area      area_expect.case's fields
    status    .by[threshold]: status_expect.case's fields       tactics   .planes [B, 3, N, N]
    patterns  .by[name of last_variants]: uint8 [B, 2, N, N]    priors    .by[(name of PRIORS, name of last_variants)]: int32 [B, N*N, 2]
    eyes      .mask [B, N, N]"""
    assert form in FORMS and family in FAMILIES
    if family not in READS_PLANE_3 and form != 'genuine':
        return expectation(N, 'genuine', family)
    B = len(boards(N).kind)
    get = lambda fn: _per_board(fn, N, form)
    if family == 'features':
        return _frozen(_merge(get(_features), _per_board(_libs, N, 'genuine')))
    if family == 'life':
        return get(_life)
    if family == 'ladder':
        rows = ladder_subset(N)
        return _frozen(_merge(_per_board(_ladder, N, form, tuple(int(r) for r in rows)), SimpleNamespace(rows=rows)))
    if family == 'outcome':
        return get(_outcome)
    if family == 'hash':
        return _frozen(_merge(get(_move_hashes), _per_board(_hashes, N, 'genuine')))
    if family == 'area':
        return get(_area)
    if family == 'status':
        return SimpleNamespace(by={thr: status_of(N, thr) for thr in se.THRESHOLDS})
    if family == 'tactics':
        return get(_tactics)
    if family == 'eyes':
        return get(_eyes)
    s = states_of(N, form)
    if family == 'patterns':
        by = {name: np.stack(mq.pattern_sets(s, last), axis=1).astype(np.uint8) for name, last in last_variants(N, B)}
    else:
        by = {(wn, ln): mpr.prior_pairs(s, last, w).astype(np.int32) for wn, w in PRIORS for ln, last in last_variants(N, B)}
    for v in by.values():
        v.setflags(write=False)
    return SimpleNamespace(by=by)


def oriented_ladder(N, form):
    """(planes, aborted) of the rows of ladder_subset(N) TURNED into the views mixed(len(rows)), then searched"""
    c = _per_board(_ladder, N, form, tuple(int(r) for r in ladder_subset(N)), True)
    return c.planes, c.aborted


@functools.lru_cache(maxsize=None)
def case(N, form):
    """every family of expectation(N, form, ...) under its name"""
    return SimpleNamespace(N=N, form=form, boards=boards(N), states=states_of(N, form),
                           **{f: expectation(N, form, f) for f in FAMILIES})


# ---------------------------------------------------------------- the playout policies
ROLLOUTS = {'no_eye_fill': mp.policy_rollout, 'tactical': mt.tactical_rollout, 'pattern': mq.pattern_rollout}


def generators(B):
    """board b of a launch of any batch size draws from generator (flood_cases.SEED, b): gogame.rng_seed(B, SEED, 0)"""
    from oracle import c_oracle
    return c_oracle.rng_seed(fc.SEED, B)


def last_before(policy, N, B):
    """the previous actions a launch starts from: the pattern policy reads them (mc_pattern_expect.last_cycle's), the others do not"""
    return mq.last_cycle(N, B) if policy == 'pattern' else np.full(B, -9, np.int32)


@functools.lru_cache(maxsize=None)
def rollout(N, policy, B, plies, auto_reset):
    """the first B boards of flood_cases.batch(N) after `plies` plies of `policy` -> (states, generators, last actions), read only"""
    start = fc.batch(N).states[:B]
    kw = {'last': last_before(policy, N, B)} if policy == 'pattern' else {}
    states, rng, last, _ = ROLLOUTS[policy](start, generators(B), plies, auto_reset, **kw)
    for a in (states, rng, last):
        a.setflags(write=False)
    return states, rng, last


@functools.lru_cache(maxsize=None)
def playout_roots(N):
    """one board of each kind ('random' too) and colour to move from the genuine form -> (rows of boards(N), states)"""
    b = boards(N)
    first = {}
    for i, k in enumerate(b.kind):
        first.setdefault((k, int(b.genuine[i, 2, 0, 0])), i)
    rows = np.array(sorted(first.values()), np.int64)
    return rows, b.genuine[rows]


@functools.lru_cache(maxsize=None)
def playouts(N, policy):
    """mc_expect.expected_playouts of playout_roots(N): PLAYOUTS playouts of at most PLAYOUT_PLIES plies, with ownership"""
    out = mc.expected_playouts(playout_roots(N)[1], PLAYOUTS, PLAYOUT_PLIES, with_ownership=True, rollout=ROLLOUTS.get(policy))
    for v in out.values():
        v.setflags(write=False)
    return out
