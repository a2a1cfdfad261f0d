"""-m gpu: the front of k_rollout5's ply (gymgo_amd/csrc/gg_v5_kernel.h, phases 1 / 2a) on crafted positions, every launch checked
against the pinned C oracle: the drawn point q travels through the ply as (row << 5) | column, a job descriptor carries its seed that
way, and phase 2a looks at q's four neighbours - at rows -1 and N and columns -1 and N when q lies on an edge - on boards that move,
pass, end, are reset and stay frozen side by side in one wave.  (The reset, frozen and pass boards were drawn for a version of phase
2a that read the neighbour rows before a finished board's planes were zeroed, docs/history/r20.md; they stay for whoever moves
those reads again.)

X is the mover's colour, Y the opponent's, q a point the first ply is forced onto (the invalid-move plane leaves only the q's of a
board and the pass); every position is run with black and with white to move.  The boards of a batch, side by side in every wave:
  (a) (e)  NEIGHBOUR boards: ten q's - the four corners, the middle of the first and last row, the first and last column on the
           two rows of the lane pair's seam (RPL - 1 and RPL), and two interior points on those rows - so that "row -1", "row N",
           "column -1" and "column N" are all read and row and column differ.  Every on-board side of every q holds what one
           pattern says: X, a Y stone with liberties, a Y stone whose only liberty is q (the capture's seed lies above / below /
           left / right of q) or nothing; the patterns are two base patterns in all four rotations and their mirror images.
  (b) (c)  FINISHED boards: two passes behind a position with stones next to almost every point.  With auto_reset the ply draws on
           the EMPTY board - a read of the neighbour rows from before the planes are zeroed would post jobs for the old stones;
           without it the board is frozen beside live ones.
  (c) (d)  PASS boards: every point invalid, so the pass is the only choice, next to boards that move - one fresh (it passes and
           plays on) and one behind a pass (it ends on the first ply of the launch: frozen from the second, or reset there).
The case `jobs` is the position of tests/test_gpu_r5.py whose first ply posts more than 64 flood jobs in a wave, so that a second
batch reads the descriptors; `pol` sends the 19x19 boards through k_rollout5_pol (policy='no_eye_fill', tracked boards) against
tests/mc_policy_expect.py.
check_boards replays every q by the rules before the GPU is touched: the move is legal, every group on the board has a liberty,
the drawing holds what its pattern says, and over the set every direction is a captured one and a friendly one and every q has all
its on-board sides occupied somewhere.  Two launches of 8 plies, the crafted ply first, with and without auto_reset, on a library
sized for four compute units (GYMGO_AMD_CUS=4), so that 1 056 games take the kernel; byte planes and tracked boards; boards,
generator states and last actions are compared with oracle.c_oracle.
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
N = 19 if CASE in ('jobs', 'pol') else int(CASE)
P = N * N
RPL = (N + 1) // 2      # rows per lane of a board's pair: the seam lies between rows RPL - 1 and RPL
DIRS = ((-1, 0), (1, 0), (0, -1), (0, 1))   # up, down, left, right: the directions 0 .. 3 of a job

def on(p):
    return 0 <= p[0] < N and 0 <= p[1] < N

def nbrs(p):
    return [(p[0] + dr, p[1] + dc) if on((p[0] + dr, p[1] + dc)) else None for dr, dc in DIRS]

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
    """the move by the rules -> (legal, the mover's group, the directions whose group is captured)"""
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
    return bool(own_libs), own, set(caught)

# a pattern: what stands above / below / left of / right of q - X, Y (with liberties), C (a Y stone whose only liberty is q), '.'
def images(base):
    """the pattern in the four rotations and their mirror images (up, down, left, right)"""
    u, d, l, r = base
    out = []
    for _ in range(4):
        u, r, d, l = l, u, r, d          # a quarter turn
        out += [(u, d, l, r), (u, d, r, l)]
    return out

PATTERNS = []
for base in (('X', 'Y', 'C', '.'), ('C', 'X', 'Y', 'C')):
    for p in images(base):
        if p not in PATTERNS:
            PATTERNS.append(p)
assert len(PATTERNS) == 16
M1, M2 = N // 2 - (2 if N == 9 else 3), N // 2 + (2 if N == 9 else 3)
QS = [(0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1), (0, N // 2), (N - 1, N // 2), (RPL - 1, 0), (RPL, N - 1)]
if N == 19:
    QS += [(RPL - 1, M1), (RPL, M2)]   # (the smaller boards have no room for them beside the edge points of the seam rows)
if N == 9:
    QS.remove((N - 1, N - 1))          # (its drawing would share a point with that of (RPL, N - 1))

def neighbour_board(k, mover):
    """board k of the set: q number i carries pattern (k + 5 i) % 16 on the sides it has -> (state, [(q, pattern)])"""
    s = np.zeros((6, N, N), np.uint8)
    qs, cores, rings = [], [], []
    for i, q in enumerate(QS):
        pat = PATTERNS[(k + 5 * i) % len(PATTERNS)]
        core, ring = {q}, set()
        for ch, n in zip(pat, nbrs(q)):
            if n is None:
                continue
            core.add(n)
            if ch == '.':
                continue
            s[mover if ch == 'X' else 1 - mover][n] = 1
            if ch == 'C':
                for m in nbrs(n):
                    if m is not None and m != q:
                        s[mover][m] = 1
                        ring.add(m)
        qs.append((q, pat))
        cores.append(core); rings.append(ring)
    # q and its sides belong to one drawing alone (the X stones around a stone to capture may be shared)
    for i in range(len(QS)):
        for j in range(len(QS)):
            assert i == j or not (cores[i] & (cores[j] | rings[j])), (k, QS[i], QS[j])
    # a drawing that is not a position (a group without a liberty) or a q that is suicide loses the q, not the board
    keep = []
    for q, pat in qs:
        assert not s[0][q] and not s[1][q], (k, q)
        if play(s, q, mover)[0]:
            keep.append((q, pat))
    s[2] = mover
    s[3] = 1
    for q, _ in keep:
        s[3][q] = 0
    return s, keep

def check_boards(boards, mover):
    cap_dirs, friend_dirs, full, rows_cols = set(), set(), set(), set()
    for s, qs in boards:
        for plane in (0, 1):
            for p in zip(*np.nonzero(s[plane])):
                assert group(s, p)[1], p
        for q, pat in qs:
            legal, own, caught = play(s, q, mover)
            assert legal
            sides = nbrs(q)
            for d, (ch, n) in enumerate(zip(pat, sides)):
                if n is None:
                    continue
                if ch == 'X':
                    assert s[mover][n] and n in own
                    friend_dirs.add(d)
                elif ch in 'YC':
                    assert s[1 - mover][n]
                    assert (d in caught) == (group(s, n)[1] == {q})
                    if ch == 'C':
                        assert d in caught
                else:
                    assert not s[0][n] and not s[1][n]
            cap_dirs |= caught
            if all(n is None or s[0][n] or s[1][n] for n in sides):
                full.add(q)
            rows_cols.add(q)
    assert cap_dirs == {0, 1, 2, 3} and friend_dirs == {0, 1, 2, 3}, (cap_dirs, friend_dirs)
    assert full == set(QS), sorted(set(QS) - full)                    # stones on every side a q has, for every q
    assert rows_cols == set(QS)
    assert {q[0] for q in QS} >= {0, N - 1, RPL - 1, RPL} and {q[1] for q in QS} >= {0, N - 1}
    assert any(q[0] != q[1] for q in QS)

def dense(mover):
    """stones next to almost every point, every group with a liberty, `mover` to move"""
    s = np.zeros((6, N, N), np.uint8)
    for r in range(N):
        for c in range(N):
            if (3 * r + c) % 5:
                s[(r // 2 + c) % 2, r, c] = 1
    while True:   # (a group the fill left without a liberty loses its first stone)
        dead = [p for plane in (0, 1) for p in zip(*np.nonzero(s[plane])) if not group(s, p)[1]]
        if not dead:
            break
        s[:2, dead[0][0], dead[0][1]] = 0
    s[2] = mover
    return s

def passed(s, times):
    """the position `times` passes later, by the oracle (the second pass ends the game)"""
    for _ in range(times):
        s, status = c_oracle.batch_next_states(s[None].copy(), np.array([P], np.int32))
        assert not status.any()
        s = s[0]
    return s

def special_boards(mover):
    fin = passed(dense(mover), 2)
    assert fin[5].all() and int(fin[0].sum() + fin[1].sum()) > P // 2
    only_pass = np.zeros((6, N, N), np.uint8)
    only_pass[mover if N > 9 else 1 - mover, 1, 1] = 1
    only_pass[2] = mover
    only_pass[3] = 1                                  # every point invalid: the pass is the only choice
    behind_pass = passed(dense(1 - mover), 1)         # `mover` to move behind a pass: the next pass ends the game
    assert behind_pass[4].all() and not behind_pass[5].any() and behind_pass[2, 0, 0] == mover
    behind_pass[3] = 1
    return [fin, only_pass, behind_pass]

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

B = 1056
positions = {}
for mover in (0, 1):
    if CASE == 'jobs':
        s0, wn = jobs_board(mover)
        positions[mover] = (np.repeat(s0[None], B, axis=0), wn)
    else:
        nb = [neighbour_board(k, mover) for k in range(len(PATTERNS))]
        check_boards(nb, mover)
        # a wave holds 32 consecutive boards: sixteen neighbour boards, then the finished, the pass-only and the behind-a-pass
        # board among them, so every wave mixes boards that move, pass, end, are reset and stay frozen
        pool = [s for s, _ in nb] + special_boards(mover)
        positions[mover] = (np.stack([pool[b % len(pool)] for b in range(B)]), nb)

import torch
from gymgo_amd import gogame, _lib
assert _lib.lib().gg_device_cus() == 4

for mover in (0, 1):
    seed = 2000 + mover
    states, extra = positions[mover]
    rng0 = gogame.rng_seed(B, seed, 0, 'cuda').cpu().numpy().view(np.uint64).copy()
    if CASE == 'pol':
        import mc_policy_expect as mp
        for auto_reset in (True, False):
            tr = gogame.batch_track(torch.from_numpy(states).cuda())
            rng = gogame.rng_seed(B, seed, 0, 'cuda')
            want, want_rng = states.copy(), rng0.copy()
            for launch in range(2):
                la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
                gogame.batch_rollout_tracked(tr, rng, 8, auto_reset, la, policy='no_eye_fill')
                want, want_rng, want_last, _ = mp.policy_rollout(want, want_rng, 8, auto_reset)
                if launch == 0:
                    assert int(((want_last >= 0) & (want_last < P)).sum()) > B // 2
                got = gogame.batch_untrack(tr).cpu().numpy()
                bad = np.flatnonzero((got != want).reshape(B, -1).any(axis=1))
                assert len(bad) == 0, (CASE, mover, auto_reset, launch, len(bad), bad[:6].tolist())
                assert np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng), (CASE, mover, auto_reset, launch)
                assert np.array_equal(la.cpu().numpy(), want_last), (CASE, mover, auto_reset, launch)
        continue
    _, _, last1 = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), 1, True)
    if CASE == 'jobs':
        jobs = np.where(last1 < P, extra.reshape(-1)[np.minimum(last1, P - 1)], 0)
        per_wave = jobs.reshape(-1, 32).sum(axis=1)
        assert int(per_wave.max()) > 64 and int((per_wave > 64).sum()) >= 8, per_wave.tolist()
    else:
        # ply 1 by the oracle: the q's of the neighbour boards are drawn in the batch.  A board stands in it 55 times and draws one
        # of at most ten q's or the pass, so one (board, q) is missed with probability (10 / 11)^55 = 0.5 %: under one of the up to
        # 160; all but a twentieth must be there, and every q on most of its boards
        npool = len(extra) + 3
        pairs = [(k, q) for k, (_, qs) in enumerate(extra) for q, _ in qs]
        seen = [(k, q) for k, q in pairs if (last1[np.arange(k, B, npool)] == q[0] * N + q[1]).any()]
        assert len(seen) >= len(pairs) - len(pairs) // 20, (N, mover, len(seen), len(pairs))
        for q in QS:
            assert sum(1 for k, p in seen if p == q) >= 12, (N, mover, q)
    for auto_reset in ((True,) if CASE == 'jobs' else (True, False)):
        wants, w, wr = [], states.copy(), rng0.copy()
        for launch in range(2):
            w, wr, wl = c_oracle.batch_rollout_mt(w.copy(), wr.copy(), 8, auto_reset)
            wants.append((w, wr, wl))
        if CASE != 'jobs':
            fin = np.arange(B) % npool == npool - 3
            ends = np.arange(B) % npool == npool - 1
            if auto_reset:   # the finished boards were reset and played on; the board behind a pass ended and was reset
                assert (wants[0][2][fin] >= 0).all() and (wants[0][2][ends] >= 0).all()
            else:            # frozen from the start / from the second ply of the launch on
                assert (wants[0][2][fin] == -1).all() and (wants[0][0][fin] == states[fin]).all()
                assert (wants[0][2][ends] == P).all() and wants[0][0][ends][:, 5].all()
                assert (wants[1][2][ends] == -1).all()
        for tracked in (False, True):
            st = torch.from_numpy(states).cuda()
            rng = gogame.rng_seed(B, seed, 0, 'cuda')
            tr = gogame.batch_track(st) if tracked else None
            for launch, (want, want_rng, want_last) in enumerate(wants):
                la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
                if tracked:
                    gogame.batch_rollout_tracked(tr, rng, 8, auto_reset, la)
                else:
                    gogame.batch_rollout(st, rng, 8, auto_reset, la)
                got = gogame.batch_untrack(tr).cpu().numpy() if tracked else st.cpu().numpy()
                bad = np.flatnonzero((got != want).reshape(B, -1).any(axis=1))
                assert len(bad) == 0, (CASE, mover, auto_reset, tracked, launch, len(bad), bad[:6].tolist())
                assert np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng), (CASE, mover, auto_reset, tracked, launch)
                assert np.array_equal(la.cpu().numpy(), want_last), (CASE, mover, auto_reset, tracked, launch)
print('R5 NEIGHBOURS OK', CASE)
'''.replace('@ROOT@', ROOT)


@pytest.mark.parametrize('case', ['19', '13', '9', 'jobs', 'pol'])
def test_r5_neighbour_reads_and_row_col_moves(case):
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    p = subprocess.run([sys.executable, '-c', SCRIPT, case], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'R5 NEIGHBOURS OK %s' % case in p.stdout
