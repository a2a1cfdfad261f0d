"""-m gpu: k_rollout5's class patch (gymgo_amd/csrc/gg_v5.h, phase 3: captures, ko, the atari-join and the mask rule) on crafted
positions, every launch checked against the pinned C oracle.

One 19x19 position, black to move, whose first ply is forced by its invalid-move plane onto one of four points (or the pass):
  A  (10, 4) captures the single white stone (10, 3) (not a ko: (10, 5) stays empty).  It rescues a black group in atari that runs
     down column 2 from row 1 to row 17 - across the rows 9 / 10 where the two lanes of a board meet - and is not next to the new
     stone: the atari-join has to fill seventeen rows from seeds in rows 9 - 11.
  B  (3, 14) captures three single white stones at once.
  C  (10, 10) captures the single stone (10, 9) with the new stone boxed in: a ko.
  D  (15, 15) captures (15, 14) and joins the black group in atari (14, 14) - (14, 15) that the captured stone touched into G.
Half the boards hold the transposed position.  The library is sized for four compute units (GYMGO_AMD_CUS=4) so that 1 056 games
take the kernel - and the FIRST launch is 8 plies long, since k_rollout5 serves launches of 8 plies or more (gg_kernels.hip:
use_rollout5): the crafted ply is ply 1 of that launch.  The games go on for 1 and 40 plies more on genuine masks, byte planes and
tracked boards.
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
N = 19
assert _lib.lib().gg_device_cus() == 4

s0 = np.zeros((6, N, N), np.uint8)
def put(plane, pts):
    for r, c in pts:
        assert s0[0, r, c] == 0 and s0[1, r, c] == 0, (r, c)
        s0[plane, r, c] = 1
# A: the black column (1 .. 17, 2) with (9, 3), (11, 3); its only liberty (18, 2)
put(1, [(r, 1) for r in range(N)] + [(0, 2)])
put(0, [(r, 2) for r in range(1, 18)] + [(9, 3), (11, 3)])
put(1, [(r, 3) for r in range(1, 9)] + [(r, 3) for r in range(12, 18)] + [(10, 3), (9, 4), (11, 4)])
# B: three single white stones around (3, 14)
put(1, [(2, 14), (4, 14), (3, 13)])
put(0, [(1, 14), (2, 13), (2, 15), (5, 14), (4, 13), (4, 15), (3, 12)])
# C: the ko shape around (10, 10)
put(1, [(10, 9), (9, 10), (11, 10), (10, 11)])
put(0, [(9, 9), (11, 9), (10, 8)])
# D: the black pair (14, 14) - (14, 15) in atari at (15, 15), next to the white stone (15, 14) in atari there
put(0, [(14, 14), (14, 15), (16, 14), (15, 13)])
put(1, [(15, 14), (13, 14), (13, 15), (14, 13), (14, 16)])

def groups(b, w):
    """(colour, stones, liberties) of every group"""
    seen, out = np.zeros((N, N), bool), []
    for col, own in ((0, b), (1, w)):
        for r0 in range(N):
            for c0 in range(N):
                if not own[r0, c0] or seen[r0, c0]:
                    continue
                st, libs, todo = set(), set(), [(r0, c0)]
                seen[r0, c0] = True
                while todo:
                    r, c = todo.pop()
                    st.add((r, c))
                    for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
                        if 0 <= rr < N and 0 <= cc < N:
                            if own[rr, cc] and not seen[rr, cc]:
                                seen[rr, cc] = True
                                todo.append((rr, cc))
                            elif not b[rr, cc] and not w[rr, cc]:
                                libs.add((rr, cc))
                out.append((col, st, libs))
    return out
gs = groups(s0[0], s0[1])
assert all(len(l) >= 1 for _, _, l in gs)
def group_of(p):
    return next(g for g in gs if p in g[1])
assert len(group_of((5, 2))[1]) == 19 and group_of((5, 2))[2] == {(18, 2)}       # A: seventeen rows, in atari
assert group_of((10, 3))[2] == {(10, 4)} and (10, 4) not in {q for p in group_of((5, 2))[1] for q in
                                                             ((p[0] - 1, p[1]), (p[0] + 1, p[1]), (p[0], p[1] - 1), (p[0], p[1] + 1))}
assert all(group_of(p)[2] == {(3, 14)} for p in ((2, 14), (4, 14), (3, 13)))     # B
assert group_of((10, 9))[2] == {(10, 10)} and all(group_of(p)[0] == 1 for p in ((9, 10), (11, 10), (10, 11)))   # C
assert group_of((14, 14))[2] == {(15, 15)} and group_of((15, 14))[2] == {(15, 15)}   # D

moves = [(10, 4), (3, 14), (10, 10), (15, 15)]
s0[3] = 1
for r, c in moves:
    s0[3, r, c] = 0
st_t = s0.transpose(0, 2, 1).copy()
B = 1056
states = np.stack([s0 if b %% 2 == 0 else st_t for b in range(B)])
rng = gogame.rng_seed(B, 91, 0, 'cuda')
want_rng = rng.cpu().numpy().view(np.uint64).copy()
after1, _, last1 = c_oracle.batch_rollout_mt(states.copy(), want_rng.copy(), 1, True)
for (r, c), ncap in zip(moves, (1, 3, 1, 1)):
    hit = np.flatnonzero((last1 == r * N + c) & (np.arange(B) %% 2 == 0))
    assert len(hit) >= 40, (r, c, len(hit))
    assert (states[hit, 1].sum(axis=(1, 2)) - after1[hit, 1].sum(axis=(1, 2)) == ncap).all(), (r, c)
ko = np.flatnonzero((last1 == 10 * N + 10) & (np.arange(B) %% 2 == 0))
assert (after1[ko, 3, 10, 9] == 1).all()                                          # the ko point is barred
for tracked in (False, True):
    st = torch.from_numpy(states).cuda()
    rng = gogame.rng_seed(B, 91, 0, 'cuda')
    want, want_rng = states.copy(), rng.cpu().numpy().view(np.uint64).copy()
    tr = gogame.batch_track(st) if tracked else None
    for F in (8, 1, 40):
        la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
        if tracked:
            gogame.batch_rollout_tracked(tr, rng, F, True, la)
        else:
            gogame.batch_rollout(st, rng, F, True, la)
        want, want_rng, want_last = c_oracle.batch_rollout_mt(want, want_rng, F, True)
        got = gogame.batch_untrack(tr).cpu().numpy() if tracked else st.cpu().numpy()
        bad = np.flatnonzero((got != want).reshape(B, -1).any(axis=1))
        assert len(bad) == 0, (F, tracked, bad[:6].tolist())
        assert np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng), (F, tracked)
        assert np.array_equal(la.cpu().numpy(), want_last), (F, tracked)
print('R5 PATCH OK')
''' % ROOT


def test_r5_class_patch_captures_ko_and_atari_join():
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    p = subprocess.run([sys.executable, '-c', SCRIPT], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'R5 PATCH OK' in p.stdout
