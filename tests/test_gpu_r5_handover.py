"""-m gpu: the hand-over of k_rollout5's flood jobs (gymgo_amd/csrc/gg_v5_kernel.h, behind flood_jobs: every lane that hands
a group over ORs its rows, two per ds_or_b64, into the board's G block or into its collection block, and one word into the board's
info word) on crafted positions, every launch checked against the pinned C oracle.

X is the mover's colour, Y the opponent's, q the point the first ply is forced onto (the invalid-move plane leaves only the q's
of a board and the pass); each drawing is run with black and with white to move.  The gadgets:
  A           q has a friendly neighbour (a G job) and THREE opponent neighbours: one group is captured, one is left with exactly
              one liberty, one keeps two or more.  G and two opponent groups leave their lanes for ONE board in one ply, two of
              them into the same collection block; the third opponent lane hands nothing over while the lanes beside it do (a
              mixed exec mask).  The four rotations and their mirror images: every direction is the captured one and the one in
              atari somewhere in the set.
  EDGE_AT     a G and an opponent column that span the seam of the lane pair (rows RPL - 1 and RPL) and reach the LAST row, whose
              row pair ORs zero into row R; the opponent column is left with one liberty.  EDGE_CAP: it is captured.
  KEEP        a friendly neighbour and one opponent neighbour that keeps >= 2 liberties: G hands over, the collection block stays zero
  ALONE       q with no neighbour at all: no job, the G block keeps q as phase 1 left it (ALONE1: the same without a margin, 9x9)
  ALONE_CAP   q with no friendly neighbour captures a stone: the G block keeps q alone, no lane may OR into it
The second case is the position of tests/test_gpu_r5.py whose first ply posts more than 64 flood jobs in a wave (a second batch:
the wave's priority is lowered again behind a raise), with either colour to move.
check_layouts recounts every group's liberties by a flood in Python, plays every q by the rules and compares what it finds
(friendly neighbour, the opponent neighbours' liberties after the move, rows reached) with what the gadget is drawn for, so a
mis-drawn position fails before the GPU is touched.  The launch is 8 plies long with the crafted ply first, on a library sized
for four compute units (GYMGO_AMD_CUS=4), so that 1 056 games take the kernel; byte planes and tracked boards; boards, generator
states and last actions are compared with oracle.c_oracle.  Two 19x19 boards, one 13x13 and one 9x9.
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
CASE = sys.argv[1]
N = 19 if CASE == 'jobs' else int(CASE)
RPL = (N + 1) // 2      # rows per lane of a board's pair: the seam lies between rows RPL - 1 and RPL

A = ['.......',
     '..XXXX.',
     '.XYqYYL',
     '..XYXX.',
     '...Y...',
     '.......']

def turned(lines, k, mirror=False):
    w = max(len(l) for l in lines)
    g = np.array([list(l.ljust(w, '.')) for l in lines])
    if mirror:
        g = g[:, ::-1]
    return [''.join(r) for r in np.rot90(g, k)]

def edge(top, lrow, cap):
    """rows top - 1 .. N - 1 of the first three columns: q at (top, 0) over a Y column, an X column beside both"""
    rows = ['...', 'qX.']
    for r in range(top + 1, N):
        rows.append('YXX' if r in (lrow - 1, lrow + 1) or (r == lrow and cap) else ('YLX' if r == lrow else 'YX.'))
    return rows

# name: (lines, q has a friendly neighbour, min(liberties left, 2) of the opponent groups next to q)
GADGETS = {
    'KEEP': (['.X.',
              'Yq.',
              'Y..',
              '...'], True, [2]),
    'ALONE': (['...',
               '.q.',
               '...'], False, []),
    'ALONE1': (['q'], False, []),          # (the same where the board has no room for the margin)
    'ALONE_CAP': (['.X..',
                   'XYq.',
                   '.X..'], False, [0]),
}
for k in range(4):
    GADGETS['A%d' % k] = (turned(A, k), True, [0, 1, 2])
    GADGETS['AM%d' % k] = (turned(A, k, True), True, [0, 1, 2])
TOP, LROW = {19: (7, 13), 13: (4, 9), 9: (2, 5)}[N]
GADGETS['EDGE_AT'] = (edge(TOP, LROW, False), True, [1])
GADGETS['EDGE_CAP'] = (edge(TOP, LROW, True), True, [0])
LAYOUTS = {
    19: [[('EDGE_AT', 6, 0), ('A0', 0, 5), ('A1', 0, 13), ('A2', 8, 5), ('A3', 8, 13), ('KEEP', 15, 6), ('ALONE', 15, 10), ('ALONE_CAP', 15, 14)],
         [('EDGE_CAP', 6, 0), ('AM0', 0, 5), ('AM1', 0, 13), ('AM2', 8, 5), ('AM3', 8, 13), ('ALONE_CAP', 15, 6), ('KEEP', 15, 11), ('ALONE', 15, 15)]],
    13: [[('EDGE_AT', 3, 0), ('ALONE_CAP', 0, 0), ('A0', 0, 5), ('AM3', 6, 7)]],
    9: [[('EDGE_AT', 1, 0), ('A1', 0, 3), ('ALONE1', 8, 6)]],
}[N]

def nbrs(p):
    """up, down, left, right (the directions 0 .. 3 of a job), None off the board"""
    return [(r, c) if 0 <= r < N and 0 <= c < N else None for r, c in ((p[0] - 1, p[1]), (p[0] + 1, p[1]), (p[0], p[1] - 1), (p[0], p[1] + 1))]

def group(s, p):
    """stones and liberties of the group at p (planes 0 / 1 of s)"""
    col = 0 if s[0][p] else 1
    assert s[col][p]
    st, libs, todo = {p}, set(), [p]
    while todo:
        for n in nbrs(todo.pop()):
            if n is None:
                continue
            if s[col][n]:
                if n not in st:
                    st.add(n); todo.append(n)
            elif not s[1 - col][n]:
                libs.add(n)
    return st, libs

def play(s, q, mover):
    """the move by the rules -> (legal, the mover's group with its liberties, the captured groups by direction)"""
    t = s.copy()
    t[mover][q] = 1
    caught = {}
    for d, n in enumerate(nbrs(q)):
        if n is not None and t[1 - mover][n] and not group(t, n)[1]:
            caught[d] = group(t, n)[0]
    for st in caught.values():
        for p in st:
            t[1 - mover][p] = 0
    own, own_libs = group(t, q)
    return bool(own_libs), own, own_libs, caught

def draw(layout, mover):
    """the layout with X = the mover's colour (0 black, 1 white) -> state, [(gadget, q)]"""
    s = np.zeros((6, N, N), np.uint8)
    used, qs = set(), []
    for name, r0, c0 in layout:
        for i, line in enumerate(GADGETS[name][0]):
            for j, ch in enumerate(line):
                p = (r0 + i, c0 + j)
                assert 0 <= p[0] < N and 0 <= p[1] < N and p not in used, (name, p)
                used.add(p)
                if ch == 'X': s[mover][p] = 1
                elif ch == 'Y': s[1 - mover][p] = 1
                elif ch == 'q': qs.append((name, p))
                else: assert ch in '.L', ch
    s[2] = mover
    s[3] = 1
    for _, q in qs:
        s[3][q] = 0
    return s, qs

def check_layouts():
    cap_dirs, atari_dirs, names = set(), set(), set()
    for layout in LAYOUTS:
        for mover in (0, 1):
            s, qs = draw(layout, mover)
            for plane in (0, 1):
                for p in zip(*np.nonzero(s[plane])):
                    assert len(group(s, p)[1]) >= 1, (layout, p)
            for name, q in qs:
                _, friendly, want = GADGETS[name]
                around = nbrs(q)
                assert friendly == any(n is not None and s[mover][n] for n in around), name
                left, seen = [], []
                for d, n in enumerate(around):
                    if n is not None and s[1 - mover][n]:
                        st, libs = group(s, n)
                        assert q in libs and st not in seen, (name, d)     # one job per group, every one a group of its own
                        seen.append(st)
                        left.append(min(len(libs - {q}), 2))
                        if len(libs) == 1: cap_dirs.add(d)
                        if len(libs) == 2: atari_dirs.add(d)
                        if name.startswith('EDGE'):
                            assert {RPL - 1, RPL, N - 1} <= {r for r, _ in st}, name     # across the seam, down to the last row
                assert sorted(left) == want, (name, left)
                legal, own, own_libs, caught = play(s, q, mover)
                assert legal and len(caught) == want.count(0), (name, len(caught))
                assert (len(own) > 1) == friendly, name
                if name.startswith('EDGE'):
                    assert {RPL - 1, RPL, N - 1} <= {r for r, _ in own}, name
                names.add(name)
    assert names == {n for l in LAYOUTS for n, _, _ in l}
    if N == 19:
        assert cap_dirs == {0, 1, 2, 3} and atari_dirs == {0, 1, 2, 3}, (cap_dirs, atari_dirs)
        assert {'A0', 'A1', 'A2', 'A3', 'EDGE_AT', 'EDGE_CAP', 'KEEP', 'ALONE', 'ALONE_CAP'} <= names

def jobs_board(mover):
    """tests/test_gpu_r5.py's position for either colour: opponent stones on every second point except a sparse grid of holes.  An
    empty point next to a hole touches THREE one-stone opponent groups (three flood jobs), every other empty point between four
    stones is suicide: ~77 jobs per wave of 32 boards on the first ply -> (state, jobs a stone at each point posts)"""
    s = np.zeros((6, N, N), np.uint8)
    for r in range(N):
        for c in range(N):
            if (r + c) % 2 == 0 and not (r % 4 == 2 and c % 4 == 2):
                s[1 - mover, r, c] = 1
    s[2] = mover
    s[3] = 1
    wn = np.zeros((N, N), np.int64)
    for r in range(N):
        for c in range(N):
            if not s[1 - mover, r, c]:
                if play(s, (r, c), mover)[0]:
                    s[3, r, c] = 0
                wn[r, c] = sum(1 for n in nbrs((r, c)) if n is not None and s[1 - mover][n])
    legal = s[3] == 0
    assert int((legal & (wn == 3)).sum()) >= 60 and int((legal & (wn == 0)).sum()) >= 12, int(legal.sum())
    assert not (legal & (wn == 4)).any()
    return s, wn

if CASE != 'jobs':
    check_layouts()

import torch
from gymgo_amd import gogame, _lib
from oracle import c_oracle
assert _lib.lib().gg_device_cus() == 4

B = 1056
for mover in (0, 1):
    seed = 1900 + mover
    rng0 = gogame.rng_seed(B, seed, 0, 'cuda').cpu().numpy().view(np.uint64).copy()
    if CASE == 'jobs':
        s0, wn = jobs_board(mover)
        states = np.repeat(s0[None], B, axis=0)
        _, _, last1 = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), 1, True)
        jobs = np.where(last1 < N * N, wn.reshape(-1)[np.minimum(last1, N * N - 1)], 0)
        per_wave = jobs.reshape(-1, 32).sum(axis=1)
        assert int(per_wave.max()) > 64 and int((per_wave > 64).sum()) >= 8, per_wave.tolist()
    else:
        drawn = [draw(layout, mover) for layout in LAYOUTS]
        states = np.stack([drawn[b % len(drawn)][0] for b in range(B)])
        # ply 1 by the oracle: every q is drawn on enough boards, a captured group leaves the board whole, any other stays
        after1, _, last1 = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), 1, True)
        for k, (s, qs) in enumerate(drawn):
            on = np.arange(k, B, len(drawn))
            for name, q in qs:
                hit = on[last1[on] == q[0] * N + q[1]]
                assert len(hit) >= 8, (N, mover, name, len(hit))
                caught = play(s, q, mover)[3]
                for d, n in enumerate(nbrs(q)):
                    if n is not None and s[1 - mover][n]:
                        for b in hit[:4]:
                            assert all(after1[b][1 - mover][p] == (0 if d in caught else 1) for p in group(s, n)[0]), (N, mover, name, int(b))
    want, want_rng, want_last = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), 8, True)
    for tracked in (False, True):
        st = torch.from_numpy(states).cuda()
        rng = gogame.rng_seed(B, seed, 0, 'cuda')
        tr = gogame.batch_track(st) if tracked else None
        la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
        if tracked:
            gogame.batch_rollout_tracked(tr, rng, 8, True, la)
        else:
            gogame.batch_rollout(st, rng, 8, True, la)
        got = gogame.batch_untrack(tr).cpu().numpy() if tracked else st.cpu().numpy()
        bad = np.flatnonzero((got != want).reshape(B, -1).any(axis=1))
        assert len(bad) == 0, (CASE, mover, tracked, len(bad), bad[:6].tolist())
        assert np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng), (CASE, mover, tracked)
        assert np.array_equal(la.cpu().numpy(), want_last), (CASE, mover, tracked)
print('R5 HANDOVER OK', CASE)
'''.replace('@ROOT@', ROOT)


@pytest.mark.parametrize('case', ['19', '13', '9', 'jobs'])
def test_r5_handover_crafted_positions(case):
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    p = subprocess.run([sys.executable, '-c', SCRIPT, case], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'R5 HANDOVER OK %s' % case in p.stdout
