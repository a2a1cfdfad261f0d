"""The area ownership planes (gg_batch_area, gogame.batch_area_planes, gogame.batch_ownership) as their definition says them -
test infrastructure, CPU only, NumPy and SciPy.  With black stones b and white stones w: E = the empty points, a REGION is a
component of E (4-neighbourhood), Rb = the regions with a point next to a black stone, Rw alike for white.  From side's view
(0 black, 1 white; None: the state's turn plane), me / op = the stones of that side / the other:
    plane 0  own_area   me | (R_me \\ R_op)
    plane 1  opp_area   op | (R_op \\ R_me)
    plane 2  neutral    E \\ (plane 0 | plane 1)
Written from that definition with scipy.ndimage.label; tests/test_area_host.py pins its counts to the oracle's batch_areas.
corridor_boards(N): the deepest flood the board allows, as own_area and as neutral."""
import functools
from collections import deque
from types import SimpleNamespace

import numpy as np
from scipy import ndimage

NAMES = ('own_area', 'opp_area', 'neutral')


def reach(stones, empty):
    """bool [N, N]: the empty points whose region has a point next to a stone of `stones`."""
    near = ndimage.binary_dilation(stones) & empty          # (the 4-neighbourhood is the default structure)
    labels, _ = ndimage.label(empty)
    hit = np.unique(labels[near])
    return np.isin(labels, hit[hit > 0])


def area_planes(state, side=None):
    """uint8 [3, N, N] of one state [6, N, N]; side: 0 black's view, 1 white's, None the state's own turn."""
    b, w = state[0] != 0, state[1] != 0
    empty = ~(b | w)
    rb, rw = reach(b, empty), reach(w, empty)
    ob, ow = b | (rb & ~rw), w | (rw & ~rb)
    white = bool(state[2, 0, 0]) if side is None else bool(side)
    me, op = (ow, ob) if white else (ob, ow)
    return np.stack([me, op, empty & ~(me | op)]).astype(np.uint8)


def batch_area_planes(states, side=None):
    """uint8 [B, 3, N, N]; side: None, one flag for all boards, or B flags."""
    states = np.asarray(states)
    sides = [None] * len(states) if side is None else np.broadcast_to(np.asarray(side), (len(states),))
    N = states.shape[-1]
    return np.stack([area_planes(s, v) for s, v in zip(states, sides)]) if len(states) else np.zeros((0, 3, N, N), np.uint8)


def counts(planes):
    """int32 [B, 2] of planes [B, 3, N, N] (or int32 [2] of [3, N, N]): the points of plane 0 and of plane 1."""
    return planes[..., :2, :, :].sum(axis=(-2, -1)).astype(np.int32)


def owner(planes):
    """(owner int8 [B, N, N] = plane 0 - plane 1, margin int32 [B] = counts[:, 0] - counts[:, 1])"""
    c = counts(planes)
    return planes[..., 0, :, :].astype(np.int8) - planes[..., 1, :, :].astype(np.int8), (c[..., 0] - c[..., 1]).astype(np.int32)


# ---------------------------------------------------------------- the deepest flood the board allows
def corridor_of(state, seed):
    """point -> steps from `seed` along the empty region that holds it (breadth first)"""
    import flood_cases as fc
    N = state.shape[-1]
    assert not state[0][seed] and not state[1][seed], seed
    dist, todo = {seed: 0}, deque([seed])
    while todo:
        p = todo.popleft()
        for n in fc.neighbours(p, N):
            if n not in dist and not state[0][n] and not state[1][n]:
                dist[n] = dist[p] + 1
                todo.append(n)
    return dist


@functools.lru_cache(maxsize=None)
def corridor_boards(N):
    """The `corridor` boards of flood_cases.cases(N) - a snake-shaped empty region inside a ring of one colour, in all eight
    orientations and with either colour as the ring - as `plain`, and each of them again with ONE stone of the other colour on
    the corridor point farthest along the corridor from q's end of it (`seed`: the corridor point next to q) as `stone`.  On a
    plain board the whole corridor is the ring colour's area; on the other the flood from the lone stone has to run the full
    length of the snake before every other corridor point is neutral.  Below 5x5 the gadget degenerates: a plain board is
    kept as flood_cases keeps it, its second form only if the corridor has a second point (the stone then has a liberty).
    -> states uint8 [K, 6, N, N], ring int32 [K] (the ring's colour), seed int32 [K, 2], far int32 [K, 2] (the lone stone,
    -1 on plain boards), corridor bool [K, N, N] (its empty points), plain bool [K].  Read only."""
    import flood_cases as fc
    c = fc.cases(N)
    rows = []
    for i, kind in enumerate(c.kind):
        if kind != 'corridor':
            continue
        s, seed = c.states[i], (int(c.seed[i][0]), int(c.seed[i][1]))
        ring = 1 - int(s[2, 0, 0])                  # the side that has just captured the snake
        dist = corridor_of(s, seed)
        region = np.zeros((N, N), bool)
        for p in dist:
            region[p] = True
        rows.append((s, ring, seed, (-1, -1), region, True))
        far = max(dist, key=lambda p: (dist[p], p))
        if far == seed:
            continue
        t = s.copy()
        t[1 - ring][far] = 1
        t[3][far] = 1
        region = region.copy()
        region[far] = False
        rows.append((t, ring, seed, far, region, False))
    if not rows:
        z = np.zeros((0, 2), np.int32)
        return SimpleNamespace(states=np.zeros((0, 6, N, N), np.uint8), ring=np.zeros(0, np.int32), seed=z, far=z,
                               corridor=np.zeros((0, N, N), bool), plain=np.zeros(0, bool))
    out = SimpleNamespace(states=np.stack([r[0] for r in rows]), ring=np.array([r[1] for r in rows], np.int32),
                          seed=np.array([r[2] for r in rows], np.int32), far=np.array([r[3] for r in rows], np.int32),
                          corridor=np.stack([r[4] for r in rows]), plain=np.array([r[5] for r in rows]))
    for v in vars(out).values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(N, kind):
    """The expectation of plane_cases.case(N, kind) (kind 'corridor': of corridor_boards(N)), computed once: .states, .planes
    [B, 3, N, N] (side=None), .black and .white (side 0 / 1), .counts of each (.counts, .counts_black, .counts_white).  Read only."""
    import plane_cases as pc
    s = corridor_boards(N).states if kind == 'corridor' else pc.case(N, kind).states
    c = SimpleNamespace(N=N, kind=kind, states=s, planes=batch_area_planes(s), black=batch_area_planes(s, 0),
                        white=batch_area_planes(s, 1))
    c.counts, c.counts_black, c.counts_white = counts(c.planes), counts(c.black), counts(c.white)
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def mixed_side(B):
    """uint8 [B]: both views in every wave, independent of the boards' own turn flags (plane_cases alternates those by b % 2)"""
    return ((np.arange(B) * 5 // 3) % 2).astype(np.uint8)
