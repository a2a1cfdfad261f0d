"""-m gpu: the job loop of k_rollout5 and phase 3's atari-join (gymgo_amd/csrc/gg_v5_kernel.h): at 19x19 a job lane reads the rows
of M of its board out of an LDS plane that the load, the reset path and the end of phase 3 keep equal to the board lanes' registers
(gg_v5.h: GG_AB_MPLANE1), and the atari-join forms the shifts of all its rows in front of the rows' chains (GG_AB_SHL1).  Crafted
batches, every launch checked against the pinned C oracle - boards, generator states, last actions and played counters.

X is the mover's colour, Y the opponent's, q a point the first ply is forced onto (the invalid-move plane leaves only the q's of a
board and the pass); each batch is run with black and with white to move, 8 plies, auto_reset on and off, tracked boards and byte
planes - the latter without a workspace, with a zero workspace (every board with stones misses) and with one that holds the batch
(every board hits: its M comes from there).  The library is sized for four compute units (GYMGO_AMD_CUS=4), where 513, 545 and 1 056
games put 18 boards into a wave and leave a last wave of 9, 5 and 12 boards, and 1 000 games put 32 into a wave and 8 into the last.

Cases '19', '13', '9' - the batch cycles through these kinds of board (13x13 and 9x9: the same batch with the gadgets that fit;
their kernels read M by ds_bpermute as before, the cases pin what the shared body does there):
  JOIN      (a, f) the only move captures a stone whose neighbour H, a mover's group with ONE liberty, now has two: H joins M in
            phase 3 by the atari-join, seeded at its foot.  H is a column across the seam of the lane pair (rows RPL - 1 and RPL) with
            a tail of four stones along a row - the join grows one stone per trip along a row: at least five trips.  The later
            plies are drawn: the rest of the board is walled off (19x19), so that the movers come back to H, its freed liberty and
            the groups beside it - a stale plane would close a flood of G through H too early or too late.
  HAND0/1   (e) the hand-over gadgets of tests/test_gpu_r5_handover.py: G plus three opponent jobs, one captured, one left in atari,
            one kept, in all four rotations and their mirror images, and the columns across the seam down to the last row, whose
            row pair ORs zero into row R.
  GONLY     (c) every q has a friendly neighbour: the board posts a G job on the first ply after the load.  The first and the last
            board of every wave and the last board of the batch are of this kind: slots 0 and 17, with 1 000 games 0 and 31, and
            the last slot of the ragged last wave.
  FIN       (b) a finished game: reset on ply 1 (auto_reset on; else frozen), then played on from the empty board.
  ENDS      (b) a pass behind it and no valid point: it passes, the game ends inside the launch, it is reset on ply 2.
Case 'jobs' - (d) the position of tests/test_gpu_r5.py that posts more than 64 jobs in a wave of 32 boards (1 000 games): the second batch
reads the same plane.
Cases 'pol', 'tac' - the 19x19 batch on tracked boards through k_rollout5_pol and k_rollout5_tac (tests/mc_policy_expect.py,
tests/mc_tactics_expect.py).
Case 'deep' - 1 056 mid-game boards (150 plies by the oracle) played on for 200 plies: what the load put into the plane goes out of
date stone by stone.
What these cases cannot see: the plane only steers where a flood batch may end early, and a library whose phase 3 never rewrites it
passed all of them (docs/history/r29.md, section 6).  That plane and registers hold the same rows is checked row by row by
tools/exp/r5_mplane_check.py on a -DGG_AB_MCHECK build; here every launch that reads the plane is held to the oracle.
The self-checks run on the CPU before the GPU is touched: every group's liberties are recounted, every q is played by the rules
(H in atari before and with two liberties after, its rows, its tail; friendly neighbours; what is captured), and the oracle's own
plies say how many boards play next to H after the join, play a stone next to a friendly one after a reset, and end inside the launch.
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
sys.path.insert(0, '@ROOT@/tests')
import numpy as np
from oracle import c_oracle
CASE = sys.argv[1]
N = int(CASE) if CASE in ('19', '13', '9') else 19
PLIES = 200 if CASE == 'deep' else 8
P = N * N
RPL = (N + 1) // 2      # rows per lane of a board's pair: the seam lies between rows RPL - 1 and RPL
GAMMA = 0x9E3779B97F4A7C15
TAIL = 4                # stones of H along a row beyond its column

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
    """the move by the rules -> (legal, the mover's group, its liberties, the captured groups by direction, the board)"""
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
    return bool(own_libs), own, own_libs, caught, t

# ---- the gadgets
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

def join_gadget():
    """drawn from row 1 on: H = a tail of TAIL stones and a corner stone on row 2, a column below the corner over rows 3 .. RPL + 1,
    its one liberty L at the far end of the bar; below the column the Y stone C whose last liberty is q"""
    rows = ['.YYYYYY.', 'YXXXXXL.', '.YYYYXY.']
    rows += ['....YXY.'] * (RPL - 2)
    rows += ['....XYX.', '.....q..']
    return rows

def block(rows, cols, eyes):
    """a solid Y block with two one-point eyes: alive, and nothing to play inside"""
    g = [['Y'] * cols for _ in range(rows)]
    for r, c in eyes:
        g[r][c] = '.'
    return [''.join(l) for l in g]

# name: (lines, q has a friendly neighbour, min(liberties left, 2) of the opponent groups next to q)
GADGETS = {
    'KEEP': (['.X.', 'Yq.', 'Y..', '...'], True, [2]),
    'ALONE': (['...', '.q.', '...'], False, []),
    'ALONE1': (['q'], False, []),
    'ALONE_CAP': (['.X..', 'XYq.', '.X..'], False, [0]),
    'JOIN': (join_gadget(), False, [0]),
}
for k in range(4):
    GADGETS['A%d' % k] = (turned(A, k), True, [0, 1, 2])
    GADGETS['AM%d' % k] = (turned(A, k, True), True, [0, 1, 2])
TOP, LROW = {19: (7, 13), 13: (4, 9), 9: (2, 5)}[N]
GADGETS['EDGE_AT'] = (edge(TOP, LROW, False), True, [1])
GADGETS['EDGE_CAP'] = (edge(TOP, LROW, True), True, [0])
if N == 19:
    GADGETS['WALL_S'] = (block(4, 19, [(1, 3), (1, 12)]), None, None)     # rows 15 .. 18
    GADGETS['WALL_E'] = (block(14, 9, [(3, 4), (9, 4)]), None, None)      # rows 0 .. 13 of columns 10 .. 18
LAYOUTS = {
    19: {'JOIN': [('JOIN', 1, 0), ('WALL_S', 15, 0), ('WALL_E', 0, 10)],
         'HAND0': [('EDGE_AT', 6, 0), ('A0', 0, 5), ('A1', 0, 13), ('A2', 8, 5), ('A3', 8, 13), ('KEEP', 15, 6), ('ALONE', 15, 10), ('ALONE_CAP', 15, 14)],
         'HAND1': [('EDGE_CAP', 6, 0), ('AM0', 0, 5), ('AM1', 0, 13), ('AM2', 8, 5), ('AM3', 8, 13), ('ALONE_CAP', 15, 6), ('KEEP', 15, 11), ('ALONE', 15, 15)],
         'GONLY': [('EDGE_AT', 6, 0), ('A0', 0, 5), ('A1', 0, 13), ('A2', 8, 5), ('A3', 8, 13), ('KEEP', 15, 6)]},
    13: {'JOIN': [('JOIN', 1, 0)],
         'HAND0': [('EDGE_AT', 3, 0), ('ALONE_CAP', 0, 0), ('A0', 0, 5), ('AM3', 6, 7)],
         'HAND1': [('EDGE_CAP', 3, 0), ('A2', 0, 5), ('AM1', 6, 7)],
         'GONLY': [('EDGE_AT', 3, 0), ('A0', 0, 5), ('AM3', 6, 7)]},
    9: {'JOIN': [('JOIN', 1, 0)],
        'HAND0': [('EDGE_AT', 1, 0), ('A1', 0, 3), ('ALONE1', 8, 6)],
        'HAND1': [('EDGE_CAP', 1, 0), ('AM3', 0, 3)],
        'GONLY': [('EDGE_AT', 1, 0), ('A1', 0, 3)]},
}[N]
KINDS = ['JOIN', 'HAND0', 'HAND1', 'GONLY', 'FIN', 'ENDS', 'JOIN']

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
    """-> the stones of H of the JOIN board, by mover"""
    H = {}
    cap_dirs, atari_dirs = set(), set()
    for kind, layout in LAYOUTS.items():
        for mover in (0, 1):
            s, qs = draw(layout, mover)
            for plane in (0, 1):
                for p in zip(*np.nonzero(s[plane])):
                    assert len(group(s, p)[1]) >= 1, (kind, p)
            assert qs, kind
            for name, q in qs:
                _, friendly, want = GADGETS[name]
                around = nbrs(q)
                assert friendly == any(n is not None and s[mover][n] for n in around), name
                assert kind != 'GONLY' or friendly, name                         # every first move of the kind posts a G job
                left, seen = [], []
                for d, n in enumerate(around):
                    if n is not None and s[1 - mover][n]:
                        st, libs = group(s, n)
                        assert q in libs and st not in seen, (name, d)           # one job per group, every one a group of its own
                        seen.append(st)
                        left.append(min(len(libs - {q}), 2))
                        if len(libs) == 1: cap_dirs.add(d)
                        if len(libs) == 2: atari_dirs.add(d)
                        if name.startswith('EDGE'):
                            assert {RPL - 1, RPL, N - 1} <= {r for r, _ in st}, name   # across the seam, down to the last row
                assert sorted(left) == want, (name, left)
                legal, own, own_libs, caught, t = play(s, q, mover)
                assert legal and len(caught) == want.count(0), (name, len(caught))
                assert (len(own) > 1) == friendly, name
                if name.startswith('EDGE'):
                    assert {RPL - 1, RPL, N - 1} <= {r for r, _ in own}, name
                if name == 'JOIN':
                    foot = (q[0] - 2, q[1])                                      # the stone of H over the captured one
                    st, libs = group(s, foot)
                    assert s[mover][foot] and len(libs) == 1 and q not in libs, libs     # H: in atari, not next to q
                    assert list(caught) == [0] and caught[0] == {(q[0] - 1, q[1])}       # one stone dies, above q, under H's foot
                    st2, libs2 = group(t, foot)
                    assert st2 == st and len(libs2) == 2                                 # H has two liberties now: it joins M
                    rows = {r for r, _ in st}
                    assert {RPL - 1, RPL} <= rows                                        # the seam of the lane pair inside H
                    bar = sorted(c for r, c in st if r == min(rows))
                    assert len(bar) == TAIL + 1 and bar[-1] == q[1] and foot[0] == max(rows)   # a tail of four: one trip a stone
                    H[mover] = st
    if N == 19:
        assert cap_dirs == {0, 1, 2, 3} and atari_dirs == {0, 1, 2, 3}, (cap_dirs, atari_dirs)
    return H

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
    return s, wn

def passed(s, n):
    for _ in range(n):
        s = c_oracle.next_state(s, P)
    return s

def dense(mover, plies, seed):
    """a mid-game board with `mover` to move"""
    s = np.zeros((1, 6, N, N), np.uint8)
    rng = c_oracle.rng_seed(seed, 1)
    s, rng, _ = c_oracle.batch_rollout(s, rng, plies, False)
    while s[0, 2, 0, 0] != mover or s[0, 5, 0, 0] or s[0, 4, 0, 0] or not (s[0, 3] == 0).any():
        s, rng, _ = c_oracle.batch_rollout(s, rng, 1, False)
    return s[0]

def boards_per_wave(B):
    """gg_kernels.hip at four compute units (boards_per_wave5, use_rollout5)"""
    waves = (B + 31) // 32
    rounds = (waves + 31) // 32
    nb = min(32, ((B + rounds * 32 - 1) // (rounds * 32) + 1) // 2 * 2)
    assert B > 4 * (128 if N == 19 else 159), B
    return nb

def batch(mover, B):
    """-> states, the kind of every board"""
    pool = {k: draw(l, mover)[0] for k, l in LAYOUTS.items()}
    pool['FIN'] = passed(dense(mover, P // 2, 61 + mover), 2)
    assert pool['FIN'][5].all() and int(pool['FIN'][0].sum() + pool['FIN'][1].sum()) > P // 8
    behind = passed(dense(1 - mover, P // 4, 71 + mover), 1)
    assert behind[4].all() and not behind[5].any() and behind[2, 0, 0] == mover
    pool['ENDS'] = behind.copy(); pool['ENDS'][3] = 1
    nb = boards_per_wave(B)
    kind = [KINDS[b % len(KINDS)] for b in range(B)]
    for w in range((B + nb - 1) // nb):       # (c) the first and the last board of every wave, the last one ragged
        kind[w * nb] = 'GONLY'
        kind[min((w + 1) * nb, B) - 1] = 'GONLY'
        assert set(KINDS) <= set(kind[w * nb:(w + 1) * nb]) or (w + 1) * nb > B, w
    return np.stack([pool[k] for k in kind]), np.array(kind)

def check_batch(states, kind, rng0, mover, B, H):
    """what the oracle's plies do to the kinds"""
    k = lambda name: np.flatnonzero(kind == name)
    qset = {name: {q[0] * N + q[1] for _, q in draw(LAYOUTS[name], mover)[1]} for name in LAYOUTS}
    friendly_q = {q[0] * N + q[1] for name in LAYOUTS for g, q in draw(LAYOUTS[name], mover)[1] if GADGETS[g][1]}
    for auto_reset in (True, False):
        s, r = states.copy(), rng0.copy()
        near_h = np.zeros(B, bool); g_after_reset = np.zeros(B, bool); was_reset = np.zeros(B, bool)
        hmask = np.zeros((N, N), bool)
        for p in H: hmask[p] = True
        around_h = np.zeros((N, N), bool)
        for p in H:
            for n in nbrs(p):
                if n is not None and n not in H: around_h[n] = True
        for ply in range(8):
            done_before = s[:, 5, 0, 0] == 1
            turn = s[:, 2, 0, 0].astype(int)
            s2, r, last = c_oracle.batch_rollout_mt(s.copy(), r.copy(), 1, auto_reset)
            if ply == 0:
                for name in LAYOUTS:
                    idx = k(name)
                    assert all(int(l) in qset[name] or l == P for l in last[idx]), name
                    assert (last[idx] < P).sum() >= len(idx) // 4, name                     # (one q: the draw passes every second time)
                idx = k('GONLY')
                assert all(int(l) in friendly_q or l == P for l in last[idx])
                nbw = boards_per_wave(B)
                edges = [b for w in range((B + nbw - 1) // nbw) for b in (w * nbw, min((w + 1) * nbw, B) - 1)]
                assert sum(1 for b in edges if last[b] < P) >= len(edges) // 2         # (c) edge slots that post a G job on ply 1
                assert any(last[w * nbw] < P for w in range(B // nbw)) and any(last[(w + 1) * nbw - 1] < P for w in range(B // nbw))
                assert last[B - 1] < P or B != 1056, int(last[B - 1])                   # the last board of the ragged last wave
                assert (last[k('ENDS')] == P).all() and s2[k('ENDS'), 5].all()
                if auto_reset:
                    assert (last[k('FIN')] >= 0).all()
                else:
                    assert (last[k('FIN')] == -1).all() and np.array_equal(s2[k('FIN')], states[k('FIN')])
            else:
                mv = np.flatnonzero((last >= 0) & (last < P))
                rr, cc = last[mv] // N, last[mv] % N
                # (a) a stone next to H while H still stands whole in its colour
                for b, r_, c_ in zip(mv, rr, cc):
                    if kind[b] == 'JOIN' and around_h[r_, c_] and all(s[b, mover][p] for p in H):
                        near_h[b] = True
                # (b) a stone next to a friendly one on a board that was reset inside the launch
                for b, r_, c_ in zip(mv, rr, cc):
                    if was_reset[b] and any(n is not None and s[b, turn[b]][n] for n in nbrs((r_, c_))):
                        g_after_reset[b] = True
            was_reset |= done_before & (last >= 0)
            s = s2
        print('self-check', CASE, mover, B, auto_reset, 'near H', int(near_h.sum()), 'reset', int(was_reset.sum()),
              'G job after a reset', int(g_after_reset.sum()))
        if B == 1056:
            assert near_h.sum() >= (8 if N == 19 else 3), int(near_h.sum())
            if auto_reset:
                assert was_reset[k('FIN')].all() and was_reset[k('ENDS')].all()
                assert g_after_reset.sum() >= 3, int(g_after_reset.sum())
            else:
                assert not was_reset.any()

H = check_layouts() if CASE not in ('jobs', 'deep') else None
# ('jobs': 1 000 games are 32 boards per wave - with 18 no wave posts more than 64 jobs)
COUNTS = (513, 545, 1056, 1000) if CASE == '19' else ((1000,) if CASE == 'jobs' else (1056,))
batches = {}
for mover in (0, 1):
    for B in COUNTS:
        rng0 = c_oracle.rng_seed(2900 + mover, B)
        if CASE == 'deep':
            if mover:
                continue
            # mid-game boards: what the load puts into the plane goes out of date stone by stone as the launch plays on
            states, rng0, _ = c_oracle.batch_rollout_mt(np.zeros((B, 6, N, N), np.uint8), rng0.copy(), 150, True)
        elif CASE == 'jobs':
            s0, wn = jobs_board(mover)
            states = np.repeat(s0[None], B, axis=0)
            _, _, last1 = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), 1, True)
            jobs = np.where(last1 < P, wn.reshape(-1)[np.minimum(last1, P - 1)], 0)
            nbw = boards_per_wave(B)
            per_wave = [int(jobs[w:w + nbw].sum()) for w in range(0, B, nbw)]
            assert nbw == 32 and sum(1 for j in per_wave if j > 64) >= 8, per_wave
        else:
            states, kind = batch(mover, B)
            if CASE in ('19', '13', '9'):
                check_batch(states, kind, rng0, mover, B, H[mover])
        batches[(mover, B)] = (states, rng0)

import torch
from gymgo_amd import gogame, _lib
assert _lib.lib().gg_device_cus() == 4

def reference(states, rng0, auto_reset):
    if CASE == 'pol':
        import mc_policy_expect as mp
        return mp.policy_rollout(states, rng0, 8, auto_reset)
    if CASE == 'tac':
        import mc_tactics_expect as mt
        return mt.tactical_rollout(states, rng0, 8, auto_reset)
    want, want_rng, want_last = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), PLIES, auto_reset)
    # the played plies by the oracle: its generator moves by one increment per ply played
    with np.errstate(over='ignore'):
        steps = np.full(len(rng0), -1, np.int64)
        for k in range(PLIES + 1):
            steps[(rng0 + np.uint64(k) * np.uint64(GAMMA)) == want_rng] = k
    assert (steps >= 0).all()
    return want, want_rng, want_last, steps

MODES = ('tracked',) if CASE in ('pol', 'tac') else ('none', 'miss', 'hit', 'tracked')
for (mover, B), (states, rng0) in batches.items():
    for auto_reset in ((True,) if CASE == 'deep' else (True, False)):
        want, want_rng, want_last, want_steps = reference(states, rng0, auto_reset)
        for mode in MODES:
            st = torch.from_numpy(states).cuda()
            rng = torch.from_numpy(rng0.view(np.int64).copy()).cuda()
            tr = gogame.batch_track(st) if mode in ('tracked', 'hit') else None
            la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
            sd = torch.zeros((B,), dtype=torch.int64, device='cuda')
            if CASE in ('pol', 'tac'):
                gogame.batch_rollout_tracked(tr, rng, 8, auto_reset, la, sd, policy='no_eye_fill' if CASE == 'pol' else 'tactical')
            elif mode == 'tracked':
                gogame.batch_rollout_tracked(tr, rng, PLIES, auto_reset, la, sd)
            else:
                # a first call on a fresh tensor runs without a workspace; a zero workspace misses on every board with stones; a
                # tracked copy of the batch is a workspace that holds every board stone for stone, with its M
                ws = None if mode == 'none' else (torch.zeros((B, 5 * N + 1), dtype=torch.int32, device='cuda') if mode == 'miss' else tr.clone())
                gogame.batch_rollout(st, rng, PLIES, auto_reset, la, sd, workspace=ws)
            got = gogame.batch_untrack(tr).cpu().numpy() if mode == 'tracked' else st.cpu().numpy()
            tag = (CASE, mover, B, auto_reset, mode)
            bad = np.flatnonzero((got != want).reshape(B, -1).any(axis=1))
            assert len(bad) == 0, (tag, len(bad), bad[:6].tolist())
            assert np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng), tag
            assert np.array_equal(la.cpu().numpy(), want_last), tag
            assert np.array_equal(sd.cpu().numpy(), want_steps), tag
print('R5 JOBLOOP OK', CASE)
'''.replace('@ROOT@', ROOT)


@pytest.mark.parametrize('case', ['19', '13', '9', 'jobs', 'pol', 'tac', 'deep'])
def test_r5_jobloop_crafted_batches(case):
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    p = subprocess.run([sys.executable, '-c', SCRIPT, case], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'R5 JOBLOOP OK %s' % case in p.stdout
