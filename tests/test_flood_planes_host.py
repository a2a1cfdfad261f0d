"""The premises of tests/flood_plane_cases.py, on the CPU, at every board size: what keeps tests/test_gpu_flood_planes.py from
being vacuous.  Each is asserted with a plain walker (flood_cases.group, flood_cases.vertical_depth) and the C oracle's next_state,
not read back from the expectation under test: the boards are as deep as a board allows; on the capture, atari, join and suicide
boards the definitional planes say at q what the kind says; no plane family is silent on a kind it can speak about; and under each
of the three playout policies every forced board takes q on the first ply of every launch."""
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import features_expect as fe
import flood_cases as fc
import flood_plane_cases as fp
import hash_expect as he

SIZES = list(fp.SIZES)
OPP_LIBS = fe.NAMES.index('opp_libs_1')
LEGAL = fe.NAMES.index('legal')
SELF_ATARI = 8          # outcome_expect.NAMES: self_atari_1 .. self_atari_4plus


def _rows(N, *kinds):
    """(row of boards(N), forced state, genuine state, the point the board is about, a stone of the group under test, variant)"""
    b = fp.boards(N)
    return [(i, b.forced[i], b.genuine[i], tuple(int(v) for v in divmod(int(b.point[i]), N)), tuple(int(v) for v in b.seed[i]),
             int(b.variant[i])) for i in range(len(b.kind)) if b.kind[i] in kinds]


def _after(N, s, q):
    from oracle import c_oracle
    nxt, status = c_oracle.batch_next_states(s[None], np.array([q[0] * N + q[1]], np.int32))
    return nxt[0], int(status[0])


@pytest.mark.parametrize('N', SIZES)
def test_the_boards_are_the_head_of_the_batch_in_two_forms(N):
    b, c = fp.boards(N), fc.cases(N)
    K, B = len(c.kind), len(b.kind)
    assert B == -(-4 * K // 3) <= 171 and b.forced.shape == b.genuine.shape == (B, 6, N, N)
    assert np.array_equal(b.forced, fc.batch(N).states[:B])
    assert all(k == 'random' for k in b.kind[3::4]) and sorted(set(b.index[b.index >= 0].tolist())) == list(range(K))
    same = (b.forced == b.genuine).reshape(B, 6, -1).all(axis=2)
    assert same[:, [0, 1, 2, 4, 5]].all()
    assert set(np.flatnonzero(~same[:, 3]).tolist()) <= set(b.differs.tolist())
    for i in b.differs:
        assert b.kind[i] in fc.FORCED and b.q[i] == b.point[i] >= 0
        f, g = b.forced[i, 3].reshape(-1), b.genuine[i, 3].reshape(-1)
        assert f.sum() == N * N - 1 and f[b.q[i]] == 0 and g[b.q[i]] == 0                # q is legal in both forms
        assert (g[((b.genuine[i, 0] | b.genuine[i, 1]) == 1).reshape(-1)] == 1).all()
        assert np.array_equal(b.genuine[i, 3], fc.invalid_moves(b.genuine[i]))
        if N >= 5 and b.kind[i] in ('capture', 'atari'):
            assert g.sum() < f.sum(), (N, i)                                              # ... and the empty corners are, too
    rows = fp.ladder_subset(N)
    if N <= fp.LADDER_ALL_UP_TO:
        assert len(rows) == B
    else:                          # every kind, both colours to move, an unturned and a quarter-turned variant of every turned kind
        have = {(b.kind[i], int(b.forced[i, 2, 0, 0])) for i in rows}
        assert have == {(k, w) for k in set(b.kind) for w in (0, 1)}, (N, have)
        for kind in fc.TURNED:
            assert {int(b.variant[i]) for i in rows if b.kind[i] == kind} == {0, 1, 8, 9}, (N, kind)
    roots, states = fp.playout_roots(N)
    assert {(b.kind[i], int(b.genuine[i, 2, 0, 0])) for i in roots} == {(b.kind[i], int(b.genuine[i, 2, 0, 0])) for i in range(B)}
    assert len(roots) == len({b.kind[i] for i in roots}) * 2 or N < 5


def _chains(s):
    """the chains of both colours of a board [6, N, N], as sets of points"""
    seen, out = set(), []
    for plane in (0, 1):
        for p in map(tuple, np.argwhere(s[plane] == 1)):
            if p not in seen:
                stones = fc.group(s, p)[0]
                seen |= stones
                out.append(stones)
    return out


def deepest(states):
    """the greatest number of vertical / of horizontal steps inside any chain and inside any empty region of the boards, each
    counted from the chain's first point in row-major / column-major order with flood_cases.vertical_depth -> (stones, empty)"""
    best = [0, 0]
    for s in states:
        e = np.zeros_like(s)
        e[0] = (s[0] | s[1]) == 0
        for k, board in enumerate((s, e)):
            for stones in _chains(board):
                if len(stones) <= best[k]:
                    continue
                turned = {(c, r) for r, c in stones}
                best[k] = max(best[k], fc.vertical_depth(stones, min(stones)), fc.vertical_depth(turned, min(turned)))
    return tuple(best)


@pytest.mark.parametrize('N', SIZES[3:])
def test_the_boards_are_as_deep_as_the_board_allows(N):
    """The bound of test_flood_cases_host.test_the_flood_is_as_deep_as_the_board_allows, on the boards the plane kernels get."""
    bound = N - 1 if N < 9 else 2 * N
    t0 = time.time()
    stones, empty = deepest(fp.boards(N).forced)
    print('flood_plane_cases N=%d: %d boards, deepest chain %d steps, deepest empty region %d steps (bound %d), %.1f s'
          % (N, len(fp.boards(N).kind), stones, empty, bound, time.time() - t0))
    assert stones >= bound and empty >= bound, (N, stones, empty, bound)
    # ... in vertical steps of the board as it is, and in horizontal ones: both on some board of every snake kind
    seen = set()
    for i, s, g, q, seed, v in _rows(N, 'capture', 'atari', 'suicide'):
        stones = fc.group(s, seed)[0]
        if v & 1:
            stones, seed = {(c, r) for r, c in stones}, seed[::-1]
        if fc.vertical_depth(stones, seed) >= bound - 1:
            seen.add((fp.boards(N).kind[i], v & 1))
    assert len(seen) == 6, (N, seen)


@pytest.mark.parametrize('N', SIZES[1:])
def test_capture_and_atari_boards_genuine_form(N):
    import mc_tactics_expect as mt
    b = fp.boards(N)
    feat, out = fp.expectation(N, 'genuine', 'features'), fp.expectation(N, 'genuine', 'outcome')
    hashes, tac = fp.expectation(N, 'genuine', 'hash'), fp.expectation(N, 'genuine', 'tactics')
    for i, s, g, q, seed, v in _rows(N, 'capture', 'atari'):
        mover = int(g[2, 0, 0])
        snake, libs = fc.group(g, seed)
        want = 1 if b.kind[i] == 'capture' else 2
        assert len(libs) == want and q in libs and g[1 - mover][seed], (N, i, libs)
        for p in snake:                                   # every snake stone in the one- / two-liberty class
            assert feat.libs[i][p] == want and feat.planes[i, OPP_LIBS + want - 1][p] == 1, (N, i, p)
            assert feat.planes[i, OPP_LIBS:OPP_LIBS + 4, p[0], p[1]].sum() == 1
        if b.kind[i] != 'capture':
            assert out.raw[i, 1][q] == 0 and not tac.planes[i, 0][q], (N, i)
            continue
        nxt, status = _after(N, g, q)
        gone = (g[1 - mover] == 1) & (nxt[1 - mover] == 0)
        assert status == 0 and int(gone.sum()) == len(snake) and all(gone[p] for p in snake), (N, i)
        assert out.raw[i, 1][q] == len(snake), (N, i, out.raw[i, :, q[0], q[1]])
        assert hashes.moves[i, q[0] * N + q[1]] == he.hash_stones(nxt[0], nxt[1]) != hashes.hashes[i], (N, i)
        assert tac.planes[i, mt.SET_C][q] == 1, (N, i)
        assert feat.planes[i, fe.NAMES.index('capture')][q] == 1, (N, i)


@pytest.mark.parametrize('N', SIZES[1:])
def test_join_and_suicide_boards(N):
    b = fp.boards(N)
    for form in fp.FORMS:
        feat, out, hashes = (fp.expectation(N, form, f) for f in ('features', 'outcome', 'hash'))
        for i, s, g, q, seed, v in _rows(N, 'join1', 'join2'):
            nxt, status = _after(N, g, q)
            stones, libs = fc.group(nxt, q)
            want = 1 if b.kind[i] == 'join1' else 2
            assert status == 0 and len(libs) == want, (N, i, libs)
            assert tuple(out.raw[i, :3, q[0], q[1]]) == (want, 0, len(stones)), (N, form, i)
            atari = out.planes[i, SELF_ATARI:SELF_ATARI + 4, q[0], q[1]]
            assert atari.sum() == (want == 1) and (want != 1 or atari[min(len(stones), 4) - 1] == 1), (N, form, i)
        for i, s, g, q, seed, v in _rows(N, 'suicide'):
            assert np.array_equal(s, g) and _after(N, g, q)[1] != 0
            assert feat.planes[i, LEGAL][q] == 0 and not out.raw[i, :, q[0], q[1]].any(), (N, form, i)
            assert hashes.moves[i, q[0] * N + q[1]] == hashes.hashes[i], (N, form, i)


# ---------------------------------------------------------------- no family is idle
def speaks(N, form):
    """family -> bool [B]: the boards on which the family's expectation says something"""
    B = len(fp.boards(N).kind)
    e = lambda f: fp.expectation(N, form, f)
    rows = lambda a: a.reshape(B, -1).any(axis=1)
    feat, lad = e('features'), e('ladder')
    ladder = np.zeros(B, bool)
    ladder[lad.rows] = lad.planes.reshape(len(lad.rows), -1).any(axis=1)
    st = e('status').by
    return {
        'liberty classes': rows(feat.planes[:, 2:10]), 'legal, ko, capture': rows(feat.planes[:, 10:13]), 'life': rows(e('life').planes),
        'ladder': ladder, 'outcome': rows(e('outcome').planes), 'move hashes': rows(e('hash').moves != e('hash').hashes[:, None]),
        'neutral area': rows(e('area').planes[:, 2]), 'area': rows(e('area').planes[:, :2]),
        'dead or unsettled': np.logical_or.reduce([rows(c.black[:, [1, 2, 4, 5]]) for c in st.values()]),
        'tactics C': rows(e('tactics').planes[:, 0]), 'tactics E': rows(e('tactics').planes[:, 1]), 'tactics F': rows(e('tactics').planes[:, 2]),
        'patterns P': rows(e('patterns').by['cycle'][:, 0]), 'patterns L': rows(e('patterns').by['cycle'][:, 1]),
        'priors': np.logical_or.reduce([rows(v) for v in e('priors').by.values()]), 'eyes': rows(e('eyes').mask)}


ALWAYS = lambda N: True
NO_MOVE = 'the mover of a suicide board has no legal point: q and both empty corners are suicide'
ONE_COLOUR = 'a corridor board holds stones of one colour only (and the stone at q): '
# (family, kind) -> (the sizes N >= 5 at which the family has nothing to say about any board of the kind, why)
IDLE = {
    ('eyes', 'capture'): (lambda N: N % 2 == 1, 'the empty corners are the only candidates; at odd N a snake stone lies diagonal to each'),
    ('eyes', 'atari'): (lambda N: N % 2 == 1, 'as on the capture boards'),
    ('eyes', 'corridor'): (ALWAYS, 'the mover is the side whose snake has just left the board: it has no stone'),
    ('eyes', 'join1'): (ALWAYS, 'every empty point touches a stone of the ring, the opponent'),
    ('eyes', 'join2'): (ALWAYS, 'every empty point touches a stone of the ring, the opponent'),
    ('eyes', 'suicide'): (ALWAYS, 'every empty point touches a stone of the ring, the opponent'),
    ('eyes', 'shape'): (ALWAYS, 'no empty point of a spiral, serpentine or comb is enclosed by the mover alone'),
    ('ladder', 'corridor'): (ALWAYS, ONE_COLOUR + 'no chain with one or two liberties'),
    ('neutral area', 'corridor'): (ALWAYS, ONE_COLOUR + 'every empty region is its area'),
    ('patterns P', 'corridor'): (ALWAYS, ONE_COLOUR + 'no pattern of the table matches there'),
    ('tactics C', 'corridor'): (ALWAYS, ONE_COLOUR + 'no opponent chain with fewer than two liberties'),
    ('life', 'atari'): (ALWAYS, 'no chain has two vital regions'),
    ('life', 'join1'): (ALWAYS, 'no chain has two vital regions'),
    ('life', 'join2'): (ALWAYS, 'no chain has two vital regions'),
    ('tactics C', 'atari'): (ALWAYS, 'the snake has two liberties, the ring more: no opponent chain with fewer than two'),
    ('tactics C', 'join1'): (ALWAYS, 'the chain in atari is the mover\'s own: no opponent chain with fewer than two liberties'),
    ('tactics C', 'join2'): (ALWAYS, 'the chain in atari is the mover\'s own: no opponent chain with fewer than two liberties'),
}
IDLE.update({(f, 'suicide'): (ALWAYS, NO_MOVE) for f in ('legal, ko, capture', 'move hashes', 'outcome', 'priors', 'tactics C', 'tactics E',
                                                         'tactics F')})
# E asks for a legal point with two empty neighbours next to a mover's chain in atari: q of a join board has none, the other
# kinds have no such chain.  The planes of E are compared all the same: they have to stay zero.
IDLE.update({('tactics E', k): (ALWAYS, 'no legal point next to a mover\'s chain in atari has two empty neighbours')
             for k in ('capture', 'atari', 'join1', 'join2', 'corridor', 'shape')})
# L depends on where mc_pattern_expect.last_cycle puts the previous move: held to speaking on SOME crafted board of every size
ANY_KIND = ('patterns L',)


@pytest.mark.parametrize('N', SIZES[3:])
def test_no_family_is_idle(N):
    """Every plane family says something on at least one board of every crafted kind it can speak about (from 5x5 on, where the
    snake is a snake; the random positions of the batch are late ones, many of them finished games, and are held to nothing)."""
    b = fp.boards(N)
    kind = np.array(b.kind)
    for form in fp.FORMS:
        for family, on in speaks(N, form).items():
            if family in ANY_KIND:
                assert on[kind != 'random'].any(), (N, form, family)
                continue
            for k in fc.KINDS:
                excused = (family, k) in IDLE and IDLE[family, k][0](N)
                assert (on & (kind == k)).any() != excused, (N, form, family, k, 'not idle: drop the excuse' if excused else 'idle')


# ---------------------------------------------------------------- the playout policies
@pytest.mark.parametrize('N', SIZES)
def test_every_forced_board_takes_q_on_the_first_ply_under_every_policy(N):
    batch = fc.batch(N)
    for policy in fp.POLICIES:
        for B in sorted({B for B, _ in fp.ROLLOUT_CELLS}):
            _, _, last = fp.rollout(N, policy, B, 1, True)
            on = [i for i in range(B) if batch.kind[i] in fc.FORCED]
            hit = [i for i in on if last[i] == batch.q[i]]
            assert hit == on and (on or N < 3), (N, policy, B, len(hit), len(on))
            if N >= 5:
                assert {batch.kind[i] for i in on} == set(fc.FORCED)
