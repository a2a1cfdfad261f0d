"""-m gpu: the per-ply bookkeeping of k_rollout5's main path (gymgo_amd/csrc/gg_v5_kernel.h and flood_jobs in gg_v5.h: lane
constants kept through the plies, wave-wide tests as one compare, the small stores of phases 1 and 3 and the hand-over under the full
exec mask, the first visit of a sweep behind the opposite one as a bit-order flip) on crafted batches, every launch checked against
the pinned C oracle - boards, generator states, last actions and played counters.

X is the mover's colour, Y the opponent's; each batch is run with black and with white to move.

Cases '19', '13', '9' - MIXED STORE MASKS IN ONE WAVE ON ONE PLY.  The batch cycles through nine kinds of board, so neighbouring
board slots (pairs of lanes) of every wave hold, on the first ply:
  MOVE      a board with stones and plenty of valid points: it moves
  PASS      every point invalid (k == n): it passes
  PASSED    a pass behind it and valid points: it moves, or passes and ends
  PASSED2   a pass behind it and every point invalid: it passes and the game ends
  DONE      a finished game: frozen (auto_reset off: nothing of it may be written) or reset on this ply (auto_reset on)
  CAPT      the only valid point captures two stones
  KO        the only valid point captures one stone and leaves a ko (across the seam of the lane pair)
  COLS      the column gadgets below
  ARCH      the arch gadget below (19x19; smaller boards: a second CAPT)
and the slots of a wave beyond its boards are switched off: the library is sized for four compute units (GYMGO_AMD_CUS=4), where
513, 545 and 1 056 games (19x19) put 18 boards into a wave of 32 slots and leave a short last wave of 9, 5 and 12 boards.  Launches are
8 plies long with auto_reset on and off, byte planes and tracked boards: the crafted ply is ply 1, and on the later plies boards pass
twice, end, are reset or freeze next to boards that move.
Case 'flood' - FLOODS THAT TOUCH ROW 0 AND ROW N - 1 (19x19), for the sweeps' turns:
  COLS      a Y column over all rows between two X columns, q in the left X column at the top, in the middle or at the bottom: the
            opponent job is seeded at either end or in the middle and its group spans every row; captured, left in atari or left with
            two liberties.  With q in the middle the mover's group G (the X column above and below q) spans every row too.
  ARCH      a Y arch whose bar lies on row 0 and whose long leg ends on row N - 1, seeded at that foot: down + up find the leg and the bar,
            the short leg is open downwards, the part has fewer than two liberties - the batch runs on with a down sweep whose first
            row has just been filled by the up sweep; captured and left in atari.
Cases 'pol', 'tac' - the mixed batch of '19' on tracked boards through k_rollout5_pol (policy='no_eye_fill', against
tests/mc_policy_expect.py) and k_rollout5_tac (policy='tactical', against tests/mc_tactics_expect.py).
check_batch asserts on the CPU, before the GPU is touched, that every kind does on ply 1 what its name says (by the oracle) and that
every wave holds every kind; check_flood recounts the groups, replays the kernel's sweeps in Python and asserts rows, seeds and sweeps.
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
P = N * N
RPL = (N + 1) // 2      # rows per lane of a board's pair: the seam lies between rows RPL - 1 and RPL
NBW = 18                # boards per wave of the launches below (asserted against the library's sizing rule)
GAMMA = 0x9E3779B97F4A7C15

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

def draw(gadgets, mover, forced=True):
    """gadgets: (row, column, lines) with 'X' the mover's stones, 'Y' the opponent's, 'q' a point the first ply may take -> state, q's"""
    s = np.zeros((6, N, N), np.uint8)
    used, qs = set(), []
    for r0, c0, lines in gadgets:
        for i, line in enumerate(lines):
            for j, ch in enumerate(line):
                p = (r0 + i, c0 + j)
                if ch == ' ':
                    continue
                assert 0 <= p[0] < N and 0 <= p[1] < N and p not in used, p
                used.add(p)
                if ch == 'X': s[mover][p] = 1
                elif ch == 'Y': s[1 - mover][p] = 1
                elif ch == 'q': qs.append(p)
                else: assert ch in '.L', ch
    s[2] = mover
    if forced:
        s[3] = 1
        for q in qs:
            s[3][q] = 0
    else:
        s[3] = s[0] | s[1]
    for plane in (0, 1):
        for p in zip(*np.nonzero(s[plane])):
            assert len(group(s, p)[1]) >= 1, p
    return s, qs

# ---- the gadgets
KO = [' XY ',
      'XYqY',
      ' XY ']
CAPT = [' XX ',
        'XYYq',
        ' XX ']

def cols_gadget(rq, libs):
    """three columns over all rows: X (q at row rq), Y, X with `libs` points left empty beside the Y column"""
    holes = {0: [], 1: [N // 3], 2: [N // 3, N - 3]}[libs]
    return ['%sY%s' % ('q' if r == rq else 'X', 'L' if r in holes else 'X') for r in range(N)]

def arch_gadget(cap):
    """columns 0 .. 6: X | the long Y leg (all rows) | X with q at its foot | . | X | the short Y leg | X; the bar on row 0"""
    kb = N // 2
    rows = []
    for r in range(N):
        if r == 0:
            rows.append('XYYYYYX')
        elif r <= kb:
            rows.append('XYX%sXYX' % ('X' if r == 1 else '.'))
        elif r == kb + 1:
            rows.append('XYX..%s.' % ('X' if cap else 'L'))
        else:
            rows.append('XY%s....' % ('q' if r == N - 1 else 'X'))
    return rows

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
        f |= {(r, c) for c in row}
    whole, todo = {seed}, [seed]
    while todo:
        for n in nbrs(todo.pop()):
            if n in own and n not in whole:
                whole.add(n); todo.append(n)
    f, n, part = {seed}, 0, None
    while f != whole or (upto is not None and n < upto):
        for r in (range(N) if n % 2 == 0 else range(N - 1, -1, -1)):
            visit(f, r, r - 1 if n % 2 == 0 else r + 1)
        n += 1
        if n == upto:
            part = set(f)
        assert n < 40
    return n, part

def flood_layouts():
    """-> [(gadgets, [(kind, q's index, wanted liberties after the move)])]: three boards of column gadgets (every seed row with
    every outcome), one with the two arches"""
    seeds = [0, N // 2, N - 1]
    out = []
    for k in range(3):
        g = [(0, 1 + 4 * i, cols_gadget(seeds[i], (i + k) % 3)) for i in range(3)] + [(0, 13, cols_gadget(seeds[k], (k + 2) % 3))]
        out.append(g)
    out.append([(0, 1, arch_gadget(True)), (0, 10, arch_gadget(False))])
    return out

def check_flood(layouts):
    seen = set()
    for k, gadgets in enumerate(layouts):
        for mover in (0, 1):
            s, qs = draw(gadgets, mover)
            assert len(qs) == len(gadgets)
            for q in qs:
                opp = [n for n in nbrs(q) if s[1 - mover][n]]
                assert len(opp) == 1
                st, libs = group(s, opp[0])
                rows = {r for r, _ in st}
                assert q in libs and rows == set(range(N)), (k, q)                  # the opponent group touches row 0 and row N - 1
                left = min(len(libs) - 1, 2)
                own = {tuple(p) for p in zip(*np.nonzero(s[1 - mover]))}
                n, part = sweeps(own, opp[0], 2)
                pl = {x for p in part for x in nbrs(p) if not s[0][x] and not s[1][x] and x != q}
                if k < 3:
                    seen.add((q[0], left))
                    assert n <= 2, (k, q, n)                                         # a column: closed by down + up
                    fr = [x for x in nbrs(q) if s[mover][x]]
                    gst = set().union(*[group(s, x)[0] for x in fr]) | {q}
                    if q[0] == N // 2:
                        assert {0, N - 1} <= {r for r, _ in gst}, (k, q)             # G through q spans every row
                else:
                    assert q[0] == N - 1 and n == 3 and len(pl) < 2 and part != st, (k, q, n, pl)   # the run-on trip: one down sweep more
                    assert {(0, c) for c in range(q[1] - 1, q[1] + 4)} <= part       # row 0 was filled by the up sweep
                    seen.add(('arch', left))
    assert seen == {(r, l) for r in (0, N // 2, N - 1) for l in (0, 1, 2)} | {('arch', 0), ('arch', 1)}, seen

def passed(s, n):
    """s after n passes by the oracle"""
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

KINDS = ['MOVE', 'PASS', 'PASSED', 'PASSED2', 'DONE', 'CAPT', 'KO', 'COLS', 'ARCH']

def pool(mover):
    mid = dense(mover, P // 3, 31 + mover)
    only_pass = mid.copy(); only_pass[3] = 1
    behind = passed(dense(1 - mover, P // 4, 41 + mover), 1)
    assert behind[4].all() and not behind[5].any() and behind[2, 0, 0] == mover and (behind[3] == 0).any()
    behind2 = behind.copy(); behind2[3] = 1
    fin = passed(dense(mover, P // 2, 51 + mover), 2)
    assert fin[5].all() and int(fin[0].sum() + fin[1].sum()) > P // 8
    capt, _ = draw([(1, 1, CAPT)], mover)
    ko, _ = draw([(RPL - 2, 1, KO)], mover)             # q on row RPL - 1, a Y stone of the box on row RPL: across the seam
    cols, _ = draw([(0, 1, cols_gadget(N // 2, 0))] + ([(0, 5, cols_gadget(N - 1, 1))] if N > 9 else []), mover)
    arch, _ = draw([(0, 1, arch_gadget(True)), (0, 10, arch_gadget(False))], mover) if N == 19 else draw([(N - 4, N - 5, CAPT)], mover)
    return [mid, only_pass, behind, behind2, fin, capt, ko, cols, arch]

def check_batch(states, rng0, mover, B):
    """what ply 1 does to every kind, by the oracle, with auto_reset on and off; every wave of NBW boards holds every kind"""
    kind = np.arange(B) % len(KINDS)
    for w in range((B + NBW - 1) // NBW):
        have = set(kind[w * NBW:(w + 1) * NBW].tolist())
        assert len(have) == len(KINDS) or (w + 1) * NBW > B, w
    k = lambda name: np.flatnonzero(kind == KINDS.index(name))
    stones = lambda s: s[:, 0].sum(axis=(1, 2)).astype(int) + s[:, 1].sum(axis=(1, 2))
    for auto_reset in (True, False):
        a1, r1, l1 = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), 1, auto_reset)
        assert ((l1[k('MOVE')] >= 0) & (l1[k('MOVE')] < P)).sum() > len(k('MOVE')) * 3 // 4
        assert (l1[k('PASS')] == P).all() and (a1[k('PASS'), 4] == 1).all() and not a1[k('PASS'), 5].any()
        assert (l1[k('PASSED')] < P).any() and (a1[k('PASSED'), 5, 0, 0] == (l1[k('PASSED')] == P)).all()
        assert (l1[k('PASSED2')] == P).all() and a1[k('PASSED2'), 5].all()
        if auto_reset:      # reset on this ply: the empty board and one move
            assert (l1[k('DONE')] >= 0).all() and (stones(a1[k('DONE')]) <= 1).all() and (r1[k('DONE')] != rng0[k('DONE')]).all()
        else:               # frozen
            assert (l1[k('DONE')] == -1).all() and np.array_equal(a1[k('DONE')], states[k('DONE')]) and (r1[k('DONE')] == rng0[k('DONE')]).all()
        for name, gone, ko in (('CAPT', 2, False), ('KO', 1, True), ('COLS', N, False)) + ((('ARCH', None, False),) if N == 19 else ()):
            idx = k(name)
            hit = idx[l1[idx] < P]
            assert len(hit) >= len(idx) // 4, (name, len(hit), len(idx))
            d = stones(states[hit]) + 1 - stones(a1[hit])
            if gone is not None and name != 'COLS':
                assert (d == gone).all(), (name, d[:8])
            else:
                assert (d >= N).any(), (name, d[:8])                                  # a whole column (arch) leaves the board
            nko = ((a1[hit, 3] == 1) & (a1[hit, 0] == 0) & (a1[hit, 1] == 0)).sum(axis=(1, 2))
            if ko:      # the captured point is forbidden to the next mover: the only empty invalid point beside suicides
                q = np.unravel_index(int(l1[hit[0]]), (N, N))
                assert all(a1[b, 3, q[0], q[1] - 1] == 1 and a1[b, 0, q[0], q[1] - 1] == 0 and a1[b, 1, q[0], q[1] - 1] == 0 for b in hit)

layouts = None
if CASE == 'flood':
    layouts = flood_layouts()
    check_flood(layouts)

COUNTS = (513, 545, 1056) if CASE == '19' else (1056,)
batches = {}
for mover in (0, 1):
    for B in COUNTS:
        # (the rules of gg_kernels.hip at four compute units - use_rollout5: more than 128 (19x19) or 159 games per unit take the
        # kernel; boards_per_wave5: 18 boards per wave for all three counts)
        rounds = ((B + 31) // 32 + 31) // 32
        assert ((B + rounds * 32 - 1) // (rounds * 32) + 1) // 2 * 2 == NBW and B > 4 * (128 if N == 19 else 159), B
        rng0 = c_oracle.rng_seed(2700 + mover, B)
        if CASE == 'flood':
            drawn = [draw(g, mover)[0] for g in layouts]
            states = np.stack([drawn[b % len(drawn)] for b in range(B)])
            a1, _, l1 = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), 1, True)
            for j, g in enumerate(layouts):
                on = np.arange(j, B, len(layouts))
                for q in draw(g, mover)[1]:
                    assert (l1[on] == q[0] * N + q[1]).sum() >= 8, (j, q)
        else:
            pl = pool(mover)
            states = np.stack([pl[b % len(pl)] for b in range(B)])
            check_batch(states, rng0, mover, B)
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
    want, want_rng, want_last = c_oracle.batch_rollout_mt(states.copy(), rng0.copy(), 8, auto_reset)
    # the played plies by the oracle: its generator moves by one increment per ply played
    with np.errstate(over='ignore'):
        steps = np.full(len(rng0), -1, np.int64)
        for k in range(9):
            steps[(rng0 + np.uint64(k) * np.uint64(GAMMA)) == want_rng] = k
    assert (steps >= 0).all()
    return want, want_rng, want_last, steps

for (mover, B), (states, rng0) in batches.items():
    for auto_reset in ((True,) if CASE == 'flood' else (True, False)):
        want, want_rng, want_last, want_steps = reference(states, rng0, auto_reset)
        if CASE in ('19', '13', '9') and not auto_reset:
            assert (want_steps == 0).any() and (want_steps == 8).any() and ((want_steps > 0) & (want_steps < 8)).any()
        for tracked in ((True,) if CASE in ('pol', 'tac') else (False, True)):
            st = torch.from_numpy(states).cuda()
            rng = torch.from_numpy(rng0.view(np.int64).copy()).cuda()
            tr = gogame.batch_track(st) if tracked else None
            la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
            sd = torch.zeros((B,), dtype=torch.int64, device='cuda')
            if CASE in ('pol', 'tac'):
                gogame.batch_rollout_tracked(tr, rng, 8, auto_reset, la, sd, policy='no_eye_fill' if CASE == 'pol' else 'tactical')
            elif tracked:
                gogame.batch_rollout_tracked(tr, rng, 8, auto_reset, la, sd)
            else:
                gogame.batch_rollout(st, rng, 8, auto_reset, la, sd)
            got = gogame.batch_untrack(tr).cpu().numpy() if tracked else st.cpu().numpy()
            tag = (CASE, mover, B, auto_reset, tracked)
            bad = np.flatnonzero((got != want).reshape(B, -1).any(axis=1))
            assert len(bad) == 0, (tag, len(bad), bad[:6].tolist(), [KINDS[b % len(KINDS)] for b in bad[:6]])
            assert np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng), tag
            assert np.array_equal(la.cpu().numpy(), want_last), tag
            assert np.array_equal(sd.cpu().numpy(), want_steps), tag
print('R5 MAINPATH OK', CASE)
'''.replace('@ROOT@', ROOT)


@pytest.mark.parametrize('case', ['19', '13', '9', 'flood', 'pol', 'tac'])
def test_r5_mainpath_crafted_batches(case):
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    p = subprocess.run([sys.executable, '-c', SCRIPT, case], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'R5 MAINPATH OK %s' % case in p.stdout
