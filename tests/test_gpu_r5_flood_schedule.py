"""-m gpu: the flood schedule of k_rollout5 (gymgo_amd/csrc/gg_v5.h, flood_jobs: first closure test after down + up at 19x19, the
loop resumed in place while a lane is unsettled) on crafted positions, every launch checked against the pinned C oracle.

Two 19x19 layouts, black to move, whose first ply is forced by the invalid-move plane onto one of the marked points (or the pass).
Layout A - white groups next to the point, flooded from the stone that touches it:
  * a snake of four legs, seeded at the foot of its first: five sweeps (down, up, down, up, down), three after the first test; once
    in atari after the move (its other liberty under its last leg: no part short of the whole finds it), once captured;
  * the same snake with liberties all along: the part two sweeps find has two, the lane is settled while its fill is cut short -
    and it shares its wave-plies with the boards that play next to the other snakes, whose lanes sweep on three times;
  * an arch seeded at one foot (open downwards after down + up: one sweep more), in atari and captured;
  * a cup seeded at one rim (closed by down + up), in atari and captured.
Layout B - black groups in atari, with the point as their last liberty, that the new stone joins to a group of M:
  * an arch + a snake of M: the fill holds the arch after three sweeps (the weak closure) and the snake after five; G has two
    liberties after the move on one gadget and one on the other - there the lane is unsettled when the arch is in, sweeps on twice,
    and all of G, the snake included, leaves M;
  * a snake in atari + a stone of M (four sweeps to the weak closure), a cup in atari + two stones of M (two).
The self-check of the layouts (check_layouts) replays the kernel's sweeps in Python and asserts these counts.
Each layout is launched on every board of the batch, and both mixed with random mid-game boards (a wave's 32 boards then hold
settled and unsettled lanes of every kind), as byte planes and as tracked boards.  The library is sized for four compute units
(GYMGO_AMD_CUS=4) so that 1 056 games take the kernel, and the launch is 8 plies long (k_rollout5 serves launches of 8 plies or
more): the crafted ply is ply 1, the other seven run on genuine masks - the next mover's mask of ply 1 decides what they may draw.
Reference loop: gym_go/envs/go_env.py:49-81 over gym_go/gogame.py:34-87.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r'''
import sys
sys.path.insert(0, %r)
import numpy as np
import torch
from gymgo_amd import gogame, _lib
from oracle import c_oracle
assert _lib.lib().gg_device_cus() == 4
N = 19
def board(gadgets):
    """gadgets: (row, column, lines) - 'B' black, 'W' white, 'q' a point the first ply may take, anything else empty"""
    s = np.zeros((6, N, N), np.uint8)
    qs = []
    for r0, c0, lines in gadgets:
        for i, line in enumerate(lines):
            for j, ch in enumerate(line):
                r, c = r0 + i, c0 + j
                assert ch == '.' or (s[0, r, c] == 0 and s[1, r, c] == 0 and (r, c) not in qs), (r, c)
                if ch == 'B': s[0, r, c] = 1
                elif ch == 'W': s[1, r, c] = 1
                elif ch == 'q': qs.append((r, c))
    s[3] = 1
    for r, c in qs:
        s[3, r, c] = 0
    return s, qs

def nbrs(p):
    return [(r, c) for r, c in ((p[0] - 1, p[1]), (p[0] + 1, p[1]), (p[0], p[1] - 1), (p[0], p[1] + 1)) if 0 <= r < N and 0 <= c < N]

def group(s, p):
    """stones and liberties of the group at p"""
    col = 0 if s[0][p] else 1
    assert s[col][p]
    st, libs, todo = {p}, set(), [p]
    while todo:
        for n in nbrs(todo.pop()):
            if s[col][n]:
                if n not in st:
                    st.add(n); todo.append(n)
            elif not s[1 - col][n]:
                libs.add(n)
    return st, libs

def sweeps(own, seed, upto=None):
    """the kernel's flood on the stones `own` from `seed`: whole-board sweeps, alternately down and up, every visit a complete
    horizontal run fill.  Returns (sweeps until the fill is the whole group, the fill after `upto` sweeps)."""
    def visit(f, r, nb):
        row = {c for c in range(N) if (r, c) in f or ((nb, c) in f and (r, c) in own)}
        for c in sorted(row):
            for d in (-1, 1):
                k = c + d
                while 0 <= k < N and (r, k) in own and k not in row:
                    row.add(k); k += d
        # (runs reached only through a stone added above are found by the loop: it walks outward from every filled column)
        f |= {(r, c) for c in row}
    whole, todo = {seed}, [seed]
    while todo:
        for n in nbrs(todo.pop()):
            if n in own and n not in whole:
                whole.add(n); todo.append(n)
    f, n, part = {seed}, 0, None
    while f != whole or (upto is not None and n < upto):
        for r in (range(N) if n %% 2 == 0 else range(N - 1, -1, -1)):
            visit(f, r, r - 1 if n %% 2 == 0 else r + 1)
        n += 1
        if n == upto:
            part = set(f)
        assert n < 40
    return n, part

def pts(s, plane):
    return {(r, c) for r in range(N) for c in range(N) if s[plane, r, c]}

# ---- layout A: opponent (white) groups next to the point black takes
SNAKE = ['.BBBBBBB.',
         'BWWWBWWWB',
         'BWBWBWBWB',
         'BWBWWWBWB']
ARCH = ['.BBB.',
        'BWWWB',
        'BWBWB',
        'BWBWB']
CUP = ['BWBWB',
       'BWBWB',
       'BWWWB',
       '.BBB.']
A, QA = board([
    (0, 0, SNAKE + ['.qBBBBB..']),      # a snake in atari: q under the foot of its first leg, the other liberty under its last
    (0, 10, SNAKE + ['.qBBBBBB.']),     # the same snake with q as its only liberty: captured
    (6, 1, ['WWW.WWW', 'W.W.W.W', 'W.WWW.W', 'q......']),   # a snake with liberties all along: settled by the part two sweeps find
    (6, 10, ARCH + ['.q...']),          # an arch in atari, q under its left foot
    (6, 14, ['.BBB.', '.WWWB', '.WBWB', '.WBWB', '.q.B.']),   # an arch q captures (it shares the column of black stones with its neighbour)
    (12, 0, ['.q...'] + CUP),           # a cup in atari, q over its left rim
    (12, 5, ['.q.B.'] + CUP),           # a cup q captures
])
SNAKE_AT, SNAKE_CAP, SNAKE_FREE, ARCH_AT, ARCH_CAP, CUP_AT, CUP_CAP = QA
# ---- layout B: black groups in atari that the stone at q joins to a group of M
JOIN = ['.WWW.WWW.WWW.',
        'WBBBWBBBWBBBW',
        'WBWBWBWBWBWBW',
        'WBWBWBWBWBWBW',
        'WBWBqBWBBBWBW']
Bd, QB = board([
    (0, 0, JOIN + ['.W.WWW.WW....']),   # arch in atari + a snake of M with two more liberties: G has two after the move
    (7, 0, JOIN + ['.W.WWW.WWW...']),   # the same with one more liberty: G, the snake of M included, has one
    (13, 0, ['.B.......',
             '.q.WWW.W.',
             'WBWBBBWBW',
             'WBWBWBWBW',
             'WBBBWBBBW',
             '.WWW.WWW.']),              # a snake in atari, q over its first leg, a stone of M over q: two liberties and more
    (1, 14, ['.B.', '.B.', '.q.W.'] + ['WBWBW', 'WBWBW', 'WBBBW', '.WWW.']),   # a cup in atari under q, two stones of M over it
])
JOIN2, JOIN1, JOIN_SNAKE, JOIN_CUP = QB

def check_layouts():
    wa, ba = pts(A, 1), pts(A, 0)
    for s in (A, Bd):
        for plane in (0, 1):
            for p in pts(s, plane):
                assert len(group(s, p)[1]) >= 1, p
    def opp(q, seed, libs_after, need, part_libs):
        st, libs = group(A, seed)
        assert seed in nbrs(q) and q in libs and min(len(libs) - 1, 2) == libs_after, (q, libs)
        n, part = sweeps(wa, seed, 2)
        assert n == need, (q, n)
        pl = {x for p in part for x in nbrs(p) if not A[0][x] and not A[1][x] and x != q}
        assert min(len(pl), 2) == part_libs, (q, pl)
        return st
    opp(SNAKE_AT, (3, 1), 1, 5, 0)          # open after two sweeps with no liberty found: three sweeps more
    opp(SNAKE_CAP, (3, 11), 0, 5, 0)
    opp(SNAKE_FREE, (8, 1), 2, 5, 2)        # two liberties in the part: settled, cut short
    opp(ARCH_AT, (9, 11), 1, 3, 0)          # one sweep more
    opp(ARCH_CAP, (9, 15), 0, 3, 0)
    opp(CUP_AT, (13, 1), 1, 2, 1)           # closed by down + up
    opp(CUP_CAP, (13, 6), 0, 2, 0)
    bb = pts(Bd, 0)
    def join(q, atari, m, libs_after, need, need_atari):
        sa, la = group(Bd, atari)
        sm, lm = group(Bd, m)
        assert la == {q} and q in lm and len(lm) >= 2 and atari in nbrs(q) and m in nbrs(q), (q, la, lm)
        after = (lm | {x for x in nbrs(q) if not Bd[0][x] and not Bd[1][x]}) - {q}
        assert min(len(after), 2) == libs_after, (q, after)
        own = bb | {q}
        n, _ = sweeps(own, q)
        assert n == need, (q, n)
        k = 1
        while not sa <= sweeps(own, q, k)[1]:
            k += 1
        assert k == need_atari, (q, k)       # sweeps until the stones outside M are in the fill
        return sa | sm | {q}
    join(JOIN2, (4, 3), (4, 5), 2, 5, 3)
    join(JOIN1, (11, 3), (11, 5), 1, 5, 3)
    join(JOIN_SNAKE, (15, 1), (13, 1), 2, 4, 4)
    join(JOIN_CUP, (4, 15), (2, 15), 2, 2, 2)
check_layouts()

B = 1056
# random mid-game boards: 60 .. 179 plies from the empty board
mid = np.zeros((B, 6, N, N), np.uint8)
mid_rng = c_oracle.rng_seed(4711, B)
for k in range(4):
    sl = slice(k * B // 4, (k + 1) * B // 4)
    mid[sl], mid_rng[sl], _ = c_oracle.batch_rollout_mt(mid[sl], mid_rng[sl], 60 + 40 * k, True)
assert 40 < (mid[:, 0] | mid[:, 1]).sum(axis=(1, 2)).mean() < 200

def stones_gone(before, after, st, plane):
    return all(before[plane][p] == 1 and after[plane][p] == 0 and after[1 - plane][p] == 0 for p in st)

def batches():
    yield 'A', np.stack([A] * B), {b: 'A' for b in range(B)}
    yield 'B', np.stack([Bd] * B), {b: 'B' for b in range(B)}
    mix = mid.copy()
    kind = {}
    for b in range(B):
        if b %% 3 != 2:
            mix[b] = A if b %% 3 == 0 else Bd
            kind[b] = 'A' if b %% 3 == 0 else 'B'
    yield 'mix', mix, kind

for name, states, kind in batches():
    rng0 = gogame.rng_seed(B, 577, 0, 'cuda').cpu().numpy().view(np.uint64).copy()
    # what ply 1 does, by the oracle: every marked point is drawn on enough boards, the captured groups leave the board whole,
    # the joined group holds the arch and the far end of the snake with the liberties the layout says (the launches below are
    # compared with the oracle stone for stone and mask for mask: the next mover's mask is plane 3 of ply 1, and ply 2 draws on it)
    after1, _, last1 = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), 1, True)
    for lay, qs in (('A', QA), ('B', QB)):
        on = np.array([b for b in range(B) if kind.get(b) == lay], dtype=np.int64)
        for q in qs:
            if len(on):
                hit = on[last1[on] == q[0] * N + q[1]]
                assert len(hit) >= 20, (name, q, len(hit))
    for q, seed in ((SNAKE_CAP, (3, 11)), (ARCH_CAP, (9, 15)), (CUP_CAP, (13, 6))):
        st = group(A, seed)[0]
        for b in [b for b in range(B) if kind.get(b) == 'A' and last1[b] == q[0] * N + q[1]]:
            assert stones_gone(states[b], after1[b], st, 1), (name, q, b)
    for q, libs, far in ((JOIN2, 2, (4, 11)), (JOIN1, 1, (11, 11))):
        for b in [b for b in range(B) if kind.get(b) == 'B' and last1[b] == q[0] * N + q[1]][:4]:
            g, l = group(after1[b], q)          # (planes 0 / 1 are black / white whoever is to move)
            assert far in g and (q[0], q[1] - 1) in g and min(len(l), 2) == libs, (name, q, b, l)
    for tracked in (False, True):
        st = torch.from_numpy(states).cuda()
        rng = gogame.rng_seed(B, 577, 0, 'cuda')
        tr = gogame.batch_track(st) if tracked else None
        la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
        if tracked:
            gogame.batch_rollout_tracked(tr, rng, 8, True, la)
        else:
            gogame.batch_rollout(st, rng, 8, True, la)
        want, want_rng, want_last = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), 8, True)
        got = gogame.batch_untrack(tr).cpu().numpy() if tracked else st.cpu().numpy()
        bad = np.flatnonzero((got != want).reshape(B, -1).any(axis=1))
        assert len(bad) == 0, (name, tracked, len(bad), bad[:6].tolist(), [kind.get(int(b)) for b in bad[:6]])
        assert np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng), (name, tracked)
        assert np.array_equal(la.cpu().numpy(), want_last), (name, tracked)
print('R5 FLOOD SCHEDULE OK')
''' % ROOT


def test_r5_flood_schedule_crafted_positions():
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    p = subprocess.run([sys.executable, '-c', SCRIPT], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'R5 FLOOD SCHEDULE OK' in p.stdout
