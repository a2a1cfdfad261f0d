"""-m gpu: the saturated liberty count of k_rollout5's flood jobs (gymgo_amd/csrc/gg_v5.h, job_liberties: the OR and the integer
SUM of the liberty rows) on crafted positions, every launch checked against the pinned C oracle.

A gadget is a group of colour X with a collar of Y stones and ONE point q whose neighbours are stones of that group and safe
Y stones only, so the stone played at q brings no liberty of its own.  The same drawing therefore serves twice: Y plays q
and the group is an OPPONENT neighbour of q, X plays q and the group is the mover's G; in both the group is left with
exactly the points marked L.  Each is run with black and with white to move.  The gadgets:
  CAP         no liberty left: captured (opponent only - for X the point is suicide)
  GCAP        no liberty left for G, which captures a stone by the move (mover only)
  ATARI       one liberty
  TWO_STONE   one liberty that touches the group at three of its stones: one bit, whatever reaches it
  COL2        two liberties in one column, adjacent rows: the sum of the rows differs from their OR, and nothing else does
  BAR         two liberties in one column, on the first and the last row of the board
  ROW2        two liberties in one row, adjacent columns
  EDGE        two liberties in the last two columns of a row
  CCC1        three liberties in the columns c, c, c + 1: their sum is a single bit
  SNAKE_AT    a snake of four legs seeded at its foot (five sweeps: resumed trips, the liberties taken behind a resumed test),
              one liberty under its last leg; SNAKE_CAP the same without it: captured (opponent only)
  BOTH        q between an arch that keeps one liberty (unsettled after down + up) and a snake with liberties all along (settled
              with its fill cut short): a settled and an unsettled lane of one board in one ply
check_layouts recounts every gadget's liberties by a flood in Python and plays q by the rules, so a mis-drawn position fails
before the GPU is touched.  The first ply is forced onto the gadgets' points (or the pass) by the invalid-move plane; the launch
is 8 plies long (k_rollout5 serves launches of 8 plies or more) on a library sized for four compute units (GYMGO_AMD_CUS=4), so
that 1 056 games take the kernel; byte planes and tracked boards; boards, masks, generator states and last actions are compared
with oracle.c_oracle.  19x19 holds every gadget on two boards; 13x13 and 9x9 hold the same set cut to size on four and six.
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
sys.path.insert(0, '@ROOT@')
import numpy as np
N = int(sys.argv[1])

def bar(n):
    mid = n // 2
    return ['.L..'] + ['YXqY' if r == mid else 'YXY.' for r in range(1, n - 1)] + ['.L..']

# name: (lines, modes - O: the group is an opponent neighbour of q, G: it is the mover's -, min(liberties left, 2) per group at q)
GADGETS = {
    'CAP': (['.YY.',
             'YXXY',
             'YXqY',
             '.YY.'], 'O', [0]),
    'GCAP': (['.YYYXX.',
              'YXXqYX.',
              '.YYYXX.'], 'G', [0]),
    'ATARI': (['.YY.',
               'YXXL',
               'YXqY',
               '.YY.'], 'OG', [1]),
    'TWO_STONE': (['.YYY.',
                   'YXXXY',
                   'YXLXY',
                   'YqYYY',
                   '.Y...'], 'OG', [1]),
    'COL2': (['.Y.',
              'YXY',
              'YXL',
              'YXL',
              'YXY',
              'YqY',
              '.Y.'], 'OG', [2]),
    'BAR': (bar(N), 'OG', [2]),
    'ROW2': (['.YLLYY.',
              'YXXXXqY',
              '.YYYYY.'], 'OG', [2]),
    'EDGE': (['.YYYYLL',
              'YqXXXXX',
              '.YYYYYY'], 'OG', [2]),
    'CCC1': (['.Y..',
              'YXY.',
              'YXL.',
              'YXY.',
              'YXL.',
              'YXY.',
              'YXXL',
              'YqY.',
              '.Y..'], 'OG', [2]),
    'SNAKE_AT': (['.YYYYYYY.',
                  'YXXXYXXXY',
                  'YXYXYXYXY',
                  'YXYXXXYXY',
                  'YqYYYYYL.',
                  '.Y'], 'OG', [1]),
    'SNAKE_CAP': (['.YYYYYYY.',
                   'YXXXYXXXY',
                   'YXYXYXYXY',
                   'YXYXXXYXY',
                   'YqYYYYYY.',
                   '.Y'], 'O', [0]),
    'BOTH': (['.YYY...',
              'YXXXY..',
              'YXYXY..',
              'YXYXY..',
              'YqY....',
              '.X.XXX.',
              '.X.X.X.',
              '.XXX.X.'], 'OG', [1, 2]),
}
LAYOUTS = {
    19: [[('BAR', 0, 0), ('SNAKE_AT', 0, 5), ('CAP', 0, 15), ('ATARI', 5, 15), ('BOTH', 7, 5), ('COL2', 10, 13), ('ROW2', 16, 5)],
         [('CCC1', 0, 0), ('SNAKE_CAP', 0, 5), ('TWO_STONE', 10, 0), ('GCAP', 6, 6), ('EDGE', 16, 12), ('SNAKE_AT', 10, 6)]],
    13: [[('BAR', 0, 0), ('SNAKE_AT', 0, 4), ('CAP', 6, 9), ('ROW2', 10, 4)],
         [('CCC1', 0, 0), ('TWO_STONE', 0, 5), ('ATARI', 6, 5), ('EDGE', 10, 6)],
         [('SNAKE_CAP', 0, 0), ('BOTH', 5, 5), ('COL2', 6, 0)],
         [('GCAP', 0, 0), ('SNAKE_AT', 4, 0), ('EDGE', 10, 6), ('COL2', 0, 10)]],
    9: [[('BAR', 0, 0), ('CAP', 0, 5), ('ATARI', 5, 5)],
        [('COL2', 0, 0), ('CCC1', 0, 4)],
        [('SNAKE_AT', 0, 0), ('ROW2', 6, 0)],
        [('TWO_STONE', 0, 0), ('GCAP', 6, 0)],
        [('BOTH', 0, 0)],
        [('SNAKE_CAP', 0, 0), ('EDGE', 6, 2)]],
}[N]

def nbrs(p):
    return [(r, c) for r, c in ((p[0] - 1, p[1]), (p[0] + 1, p[1]), (p[0], p[1] - 1), (p[0], p[1] + 1)) if 0 <= r < N and 0 <= c < N]

def group(s, p):
    """stones and liberties of the group at p (planes 0 / 1 of s)"""
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

def draw(layout, mode, mover):
    """the layout with X / Y coloured for `mode` and `mover` (0 black, 1 white) to move -> state, [(gadget, q, marked liberties)]"""
    xcol = mover if mode == 'G' else 1 - mover
    s = np.zeros((6, N, N), np.uint8)
    used, qs = set(), []
    for name, r0, c0 in layout:
        lines, modes, want = GADGETS[name]
        q, marks = None, set()
        for i, line in enumerate(lines):
            for j, ch in enumerate(line):
                p = (r0 + i, c0 + j)
                assert 0 <= p[0] < N and 0 <= p[1] < N and p not in used, (name, p)
                used.add(p)
                if ch == 'X': s[xcol][p] = 1
                elif ch == 'Y': s[1 - xcol][p] = 1
                elif ch == 'q': q = p
                elif ch == 'L': marks.add(p)
                else: assert ch == '.', ch
        if mode in modes:
            qs.append((name, q, marks))
    s[2] = mover
    s[3] = 1
    for _, q, _ in qs:
        s[3][q] = 0
    return s, qs

def check_layouts():
    """every drawing recounted: the group's liberties are q and the marked points, the move at q is legal and leaves what the
    gadget says, for the opponent group and for G"""
    seen = set()
    for layout in LAYOUTS:
        for mode in 'OG':
            for mover in (0, 1):
                s, qs = draw(layout, mode, mover)
                for plane in (0, 1):
                    for p in zip(*np.nonzero(s[plane])):
                        assert len(group(s, p)[1]) >= 1, (layout, p)
                xcol = mover if mode == 'G' else 1 - mover
                for name, q, marks in qs:
                    want = GADGETS[name][2]
                    assert all(s[0][n] or s[1][n] for n in nbrs(q)), (name, q)       # the stone at q brings no liberty of its own
                    xg = []
                    for n in nbrs(q):
                        if s[xcol][n] and not any(n in g[0] for g in xg):
                            xg.append(group(s, n))
                    left = [g[1] - {q} for g in xg]
                    if name != 'GCAP':
                        assert sorted(min(len(l), 2) for l in left) == want, (name, mode, left)
                        if len(xg) == 1:
                            assert left[0] == marks, (name, mode, left, marks)
                    t = s.copy()
                    t[mover][q] = 1
                    own, own_libs = group(t, q)
                    caught = []
                    for n in nbrs(q):
                        if t[1 - mover][n] and not any(n in g[0] for g in caught) and not group(t, n)[1]:
                            caught.append(group(t, n))
                    assert own_libs or caught, (name, mode, 'suicide')
                    if mode == 'G':
                        assert min(len(own_libs), 2) == (0 if name == 'GCAP' else max(want)), (name, own_libs)
                        assert (name == 'GCAP') == bool(caught), name
                        assert all(st <= own for st, _ in xg)
                    else:
                        assert len(caught) == want.count(0) and own_libs, (name, caught)
                    seen.add((name, mode))
    for name, (_, modes, _) in GADGETS.items():
        for mode in modes:
            assert (name, mode) in seen, (name, mode)
check_layouts()

import torch
from gymgo_amd import gogame, _lib
from oracle import c_oracle
assert _lib.lib().gg_device_cus() == 4

B = 1056
for mode in 'OG':
    for mover in (0, 1):
        drawn = [draw(layout, mode, mover) for layout in LAYOUTS]
        states = np.stack([drawn[b % len(drawn)][0] for b in range(B)])
        rng0 = gogame.rng_seed(B, 1700 + mover, 0, 'cuda').cpu().numpy().view(np.uint64).copy()
        # ply 1 by the oracle: every point is drawn on enough boards, a captured group leaves the board whole, any other stays
        after1, _, last1 = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), 1, True)
        for k, (s, qs) in enumerate(drawn):
            on = np.arange(k, B, len(drawn))
            xcol = mover if mode == 'G' else 1 - mover
            for name, q, marks in qs:
                hit = on[last1[on] == q[0] * N + q[1]]
                assert len(hit) >= 8, (N, mode, mover, name, len(hit))
                for n in nbrs(q):
                    if s[xcol][n]:
                        st, libs = group(s, n)
                        gone = mode == 'O' and libs == {q}
                        for b in hit[:4]:
                            assert all(after1[b][xcol][p] == (0 if gone else 1) for p in st), (N, mode, mover, name, int(b))
        for tracked in (False, True):
            st = torch.from_numpy(states).cuda()
            rng = gogame.rng_seed(B, 1700 + mover, 0, 'cuda')
            tr = gogame.batch_track(st) if tracked else None
            la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
            if tracked:
                gogame.batch_rollout_tracked(tr, rng, 8, True, la)
            else:
                gogame.batch_rollout(st, rng, 8, True, la)
            want, want_rng, want_last = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), 8, True)
            got = gogame.batch_untrack(tr).cpu().numpy() if tracked else st.cpu().numpy()
            bad = np.flatnonzero((got != want).reshape(B, -1).any(axis=1))
            assert len(bad) == 0, (N, mode, mover, tracked, len(bad), bad[:6].tolist())
            assert np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng), (N, mode, mover, tracked)
            assert np.array_equal(la.cpu().numpy(), want_last), (N, mode, mover, tracked)
print('R5 LIBERTIES OK', N)
'''.replace('@ROOT@', ROOT)


@pytest.mark.parametrize('size', [19, 13, 9])
def test_r5_liberties_crafted_positions(size):
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    p = subprocess.run([sys.executable, '-c', SCRIPT, str(size)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'R5 LIBERTIES OK %d' % size in p.stdout
