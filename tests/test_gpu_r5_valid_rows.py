"""-m gpu: the mask rows and the draw counter of k_rollout5's 19x19 ply (gymgo_amd/csrc/gg_v5_kernel.h; gg_v5.h: GG_AB_VALID1,
GG_AB_ALLMOVE1, GG_AB_DRAWADD1): a lane carries the VALID points of its rows from the load to the write-back (both convert once), the
reset path stands in front of the draw, phase 3 assigns the new rows when every board of the wave moves and selects otherwise, ko
clears a bit instead of setting one, and the draw's counter is a running sum.  Crafted batches, every launch checked against the
pinned C oracle - boards with their invalid plane, generator states, last actions and played counters; the policy cases against
tests/mc_policy_expect.py, tests/mc_tactics_expect.py and tests/mc_pattern_expect.py.

X is the mover's colour, Y the opponent's; a q is a point the first ply is forced onto (the invalid plane leaves only the q's of a
board and the pass).  8 plies, black and white to move, auto_reset on and off, tracked boards and byte planes - the latter without a
workspace, with a zero workspace (every board with stones misses) and with one that holds the batch (every board hits).  The library
is sized for four compute units (GYMGO_AMD_CUS=4): 1 024 and 1 000 games put 32 boards into a wave (every wave full, or the last
one short: the assigning path of phase 3), 513 and 545 games put 18 into a wave (absent slots: the select path).

The batch cycles through these kinds of board:
  KOSEAM  two ko shapes across the seam of the lane pair (rows 9 and 10): q on row 9 takes the stone on row 10 and the other way
          round - the ko bit is cleared in the partner lane's rows.
  KOEDGE  four ko shapes whose ko point lies on row 0, on row 18, on column 0 and on column 18.
          (Both: the ko point is invalid after the capture and legal again one ply later, by the oracle.)
  PASS1   no valid point: the board passes on ply 1 and plays on.
  ENDS    a pass behind it and no valid point: it passes, the game ends on ply 1; reset on ply 2 (auto_reset), else frozen from
          ply 2 on - a full wave that assigned on ply 1 selects from ply 2 on.
  PASS2   the mover passes (no valid point), the opponent has no legal point and passes too: the game ends on ply 2.
  ONLY9 / ONLY10  the only valid point lies on row 9 (the even lane's last row) / on row 10 (the odd lane's first).
  FIN     a finished game: reset on ply 1 - its draw is over the EMPTY board - or frozen with the invalid plane it came with.  (Every
          second wave holds none, so that it is full of boards that move on ply 1.)
  MOVE    a mid-game board that simply plays.
Cases '1024', '1000', '513', '545': the batch at that size.  Case 'deep': one launch of 200 plies on 1 056 mid-game boards.  Cases
'pol', 'tac', 'pat': the batch of 1 024 on tracked boards through policy='no_eye_fill', 'tactical' and 'pattern'.  Case 'log': the
same through the move-log entry point, with the log.
The self-checks run on the CPU before the GPU is touched: by the oracle's own plies every kind does on its ply what its name says.
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
N = 19
P = N * N
RPL = (N + 1) // 2      # rows per lane of a board's pair: the seam lies between rows RPL - 1 and RPL
PLIES = 200 if CASE == 'deep' else 8
GAMMA = 0x9E3779B97F4A7C15

# ---- the ko shapes: (q, the ko point, Y stones, X stones); X takes the Y stone on the ko point by playing q
def ko_shape(q, d):
    """q and the direction d = (dr, dc) of the stone it takes"""
    ko = (q[0] + d[0], q[1] + d[1])
    side = (d[1], d[0])
    ys = [ko, (q[0] - d[0], q[1] - d[1]), (q[0] + side[0], q[1] + side[1]), (q[0] - side[0], q[1] - side[1])]
    xs = [(ko[0] + d[0], ko[1] + d[1]), (ko[0] + side[0], ko[1] + side[1]), (ko[0] - side[0], ko[1] - side[1])]
    on = lambda p: 0 <= p[0] < N and 0 <= p[1] < N
    return q, ko, [p for p in ys if on(p)], [p for p in xs if on(p)]

SHAPES = {
    'KOSEAM': [ko_shape((RPL - 1, 4), (1, 0)), ko_shape((RPL, 12), (-1, 0))],
    'KOEDGE': [ko_shape((1, 5), (-1, 0)), ko_shape((N - 2, 13), (1, 0)), ko_shape((6, 1), (0, -1)), ko_shape((13, N - 2), (0, 1))],
}
assert [s[1][0] for s in SHAPES['KOSEAM']] == [RPL, RPL - 1]
assert [s[1] for s in SHAPES['KOEDGE']] == [(0, 5), (N - 1, 13), (6, 0), (13, N - 1)]
ONLY = {'ONLY9': (RPL - 1, 7), 'ONLY10': (RPL, 11)}

def forced(s, mover, qs):
    s[2] = mover
    s[3] = 1
    for q in qs:
        s[3][q] = 0
    return s

def ko_board(kind, mover):
    s = np.zeros((6, N, N), np.uint8)
    for q, ko, ys, xs in SHAPES[kind]:
        for p in ys: s[1 - mover][p] = 1
        for p in xs: s[mover][p] = 1
    assert not (s[0] & s[1]).any()
    return forced(s, mover, [sh[0] for sh in SHAPES[kind]])

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
    assert B > 4 * 128, B
    return nb

CYCLE = ['KOSEAM', 'KOEDGE', 'MOVE', 'PASS1', 'ENDS', 'PASS2', 'ONLY9', 'ONLY10', 'FIN', 'MOVE', 'KOSEAM']

def pool_of(mover):
    pool = {k: ko_board(k, mover) for k in SHAPES}
    pool['MOVE'] = dense(mover, P // 3, 81 + mover)
    pool['PASS1'] = forced(dense(mover, P // 4, 91 + mover).copy(), mover, [])
    behind = passed(dense(1 - mover, P // 4, 71 + mover), 1)
    assert behind[4].all() and not behind[5].any() and behind[2, 0, 0] == mover
    pool['ENDS'] = forced(behind.copy(), mover, [])
    two = np.zeros((6, N, N), np.uint8)      # one X group with two one-point eyes: nothing for Y to play, and X is told to pass
    two[mover] = 1
    two[mover][0, 0] = two[mover][N - 1, N - 1] = 0
    pool['PASS2'] = forced(two, mover, [])
    for k, q in ONLY.items():
        pool[k] = forced(np.zeros((6, N, N), np.uint8), mover, [q])
    pool['FIN'] = passed(dense(mover, P // 2, 61 + mover), 2)
    assert pool['FIN'][5].all() and int(pool['FIN'][0].sum() + pool['FIN'][1].sum()) > P // 8
    return pool

def batch(mover, B):
    """-> states, the kind of every board"""
    pool = pool_of(mover)
    nb = boards_per_wave(B)
    kind = []
    for b in range(B):
        k = CYCLE[(b % nb) % len(CYCLE)]
        if k == 'FIN' and (b // nb) % 2 == 0:
            k = 'MOVE'                          # every second wave: full of boards that move on ply 1
        kind.append(k)
    for w in range(B // nb):
        assert set(CYCLE) - {'FIN'} <= set(kind[w * nb:(w + 1) * nb]), w
    return np.stack([pool[k] for k in kind]), np.array(kind)

def check_batch(states, kind, rng0, mover, B):
    """what the oracle's plies do to the kinds"""
    k = lambda name: np.flatnonzero(kind == name)
    nbw = boards_per_wave(B)
    for auto_reset in (True, False):
        s, r = states.copy(), rng0.copy()
        hist, lasts = [s], []
        for ply in range(3):
            s, r, last = c_oracle.batch_rollout_mt(s.copy(), r.copy(), 1, auto_reset)
            hist.append(s); lasts.append(last)
        l1, l2, l3 = lasts
        s1, s2 = hist[1], hist[2]
        # ko: q takes one stone, the ko point is empty and invalid for the opponent; one ply later it is legal again
        again = 0
        for name, shapes in SHAPES.items():
            idx = k(name)
            qflat = {q[0] * N + q[1]: ko for q, ko, _, _ in shapes}
            assert all(int(l) in qflat or l == P for l in l1[idx]), name
            seen = set()
            for b in idx:
                if l1[b] == P:
                    continue
                ko = qflat[int(l1[b])]
                assert s1[b, 3][ko] == 1 and not s1[b, 0][ko] and not s1[b, 1][ko], (name, b, ko)
                assert int(s1[b, 1 - mover].sum()) == int(states[b, 1 - mover].sum()) - 1, (name, b)    # exactly one stone died
                assert l2[b] != ko[0] * N + ko[1]
                seen.add(ko)
                if not s2[b, 0][ko] and not s2[b, 1][ko] and s2[b, 3][ko] == 0:
                    again += 1
            assert seen == set(qflat.values()), (name, seen)       # every shape of the kind is played on some board
        assert again >= 8, again
        assert (l1[k('PASS1')] == P).all() and not s1[k('PASS1'), 5].any() and (l2[k('PASS1')] >= 0).all()
        assert (l1[k('ENDS')] == P).all() and s1[k('ENDS'), 5].all()
        assert (l1[k('PASS2')] == P).all() and not s1[k('PASS2'), 5].any()
        assert (l2[k('PASS2')] == P).all() and s2[k('PASS2'), 5].all()
        assert (l1[k('MOVE')] >= 0).all() and (l2[k('MOVE')] >= 0).all() and (l3[k('MOVE')] >= 0).all()
        for name, q in ONLY.items():
            idx = k(name)
            assert all(l in (q[0] * N + q[1], P) for l in l1[idx]) and (l1[idx] < P).sum() >= len(idx) // 4, name
        fin = k('FIN')
        if auto_reset:
            assert (l2[k('ENDS')] >= 0).all() and (l3[k('PASS2')] >= 0).all()              # reset on ply 2 / on ply 3
            pts = l1[fin][l1[fin] < P]
            assert (l1[fin] >= 0).all() and len(pts) >= len(fin) // 2
            occupied = (states[fin[0], 0] | states[fin[0], 1] | states[fin[0], 3]).reshape(-1)
            assert occupied[pts].sum() >= len(pts) // 8, int(occupied[pts].sum())         # the draw of a reset board: over the empty board
            assert all(int(s1[b, 0].sum() + s1[b, 1].sum()) == (1 if l1[b] < P else 0) for b in fin)
        else:
            assert (l2[k('ENDS')] == -1).all() and (l3[k('PASS2')] == -1).all()
            assert np.array_equal(s2[k('ENDS')], s1[k('ENDS')])
            assert (l1[fin] == -1).all() and np.array_equal(hist[3][fin], states[fin])     # frozen, with the invalid plane it came with
            # a full wave whose boards all move on ply 1 (phase 3 assigns) and not all on ply 2 (it selects)
            turns = sum(1 for w in range(B // nbw) if (l1[w * nbw:(w + 1) * nbw] >= 0).all() and (l2[w * nbw:(w + 1) * nbw] == -1).any())
            assert nbw != 32 or turns >= 8, turns
            print('self-check', CASE, mover, B, 'waves that go from assigning to selecting', turns, 'ko legal again', again)

COUNTS = (1056,) if CASE == 'deep' else ((int(CASE),) if CASE.isdigit() else (1024,))
batches = {}
for mover in (0, 1):
    for B in COUNTS:
        rng0 = c_oracle.rng_seed(3200 + mover, B)
        if CASE == 'deep':
            if mover:
                continue
            states, rng0, _ = c_oracle.batch_rollout_mt(np.zeros((B, 6, N, N), np.uint8), rng0.copy(), 150, True)
        else:
            states, kind = batch(mover, B)
            if CASE.isdigit():
                check_batch(states, kind, rng0, mover, B)
        batches[(mover, B)] = (states, rng0)

import torch
from gymgo_amd import gogame, _lib
assert _lib.lib().gg_device_cus() == 4
POLICY = {'pol': 'no_eye_fill', 'tac': 'tactical', 'pat': 'pattern'}

def reference(states, rng0, auto_reset):
    """-> boards, generator states, last actions, played plies, and (case 'log') the action of every ply played"""
    if CASE == 'pol':
        import mc_policy_expect as mp
        return mp.policy_rollout(states, rng0, PLIES, auto_reset) + (None,)
    if CASE == 'tac':
        import mc_tactics_expect as mt
        return mt.tactical_rollout(states, rng0, PLIES, auto_reset) + (None,)
    if CASE == 'pat':
        import mc_pattern_expect as mq
        return mq.pattern_rollout(states, rng0, PLIES, auto_reset) + (None,)
    log = None
    if CASE == 'log':
        log = np.full((len(rng0), PLIES), -7, np.int16)
        s, r = states.copy(), rng0.copy()
        for t in range(PLIES):
            s, r, last = c_oracle.batch_rollout_mt(s.copy(), r.copy(), 1, auto_reset)
            log[last >= 0, t] = last[last >= 0]
    want, want_rng, want_last = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), PLIES, auto_reset)
    # the played plies by the oracle: its generator moves by one increment per ply played
    with np.errstate(over='ignore'):
        steps = np.full(len(rng0), -1, np.int64)
        for k in range(PLIES + 1):
            steps[(rng0 + np.uint64(k) * np.uint64(GAMMA)) == want_rng] = k
    assert (steps >= 0).all()
    return want, want_rng, want_last, steps, log

MODES = ('none', 'miss', 'hit', 'tracked') if CASE.isdigit() else (('none', 'tracked') if CASE == 'deep' else ('tracked',))
for (mover, B), (states, rng0) in batches.items():
    for auto_reset in ((True,) if CASE == 'deep' else ((False,) if CASE == 'log' else (True, False))):
        want, want_rng, want_last, want_steps, want_log = reference(states, rng0, auto_reset)
        for mode in MODES:
            st = torch.from_numpy(states).cuda()
            rng = torch.from_numpy(rng0.view(np.int64).copy()).cuda()
            tr = gogame.batch_track(st) if mode in ('tracked', 'hit') else None
            la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
            sd = torch.zeros((B,), dtype=torch.int64, device='cuda')
            if CASE in POLICY:
                gogame.batch_rollout_tracked(tr, rng, PLIES, auto_reset, la, sd, policy=POLICY[CASE])
            elif CASE == 'log':
                log = torch.full((B, PLIES), -7, dtype=torch.int16, device='cuda')
                gogame.batch_rollout_tracked_log(tr, rng, PLIES, log, la, sd)
                assert np.array_equal(log.cpu().numpy(), want_log), (CASE, mover)
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
print('R5 VALID ROWS OK', CASE)
'''.replace('@ROOT@', ROOT)


@pytest.mark.parametrize('case', ['1024', '1000', '513', '545', 'deep', 'pol', 'tac', 'pat', 'log'])
def test_r5_valid_rows_crafted_batches(case):
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    p = subprocess.run([sys.executable, '-c', SCRIPT, case], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'R5 VALID ROWS OK %s' % case in p.stdout
