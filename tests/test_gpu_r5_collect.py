"""-m gpu: k_rollout5's collection of opponent groups (gymgo_amd/csrc/gg_v5.h, phase 2b: a group left with fewer than two
liberties is ORed into its board's collection block two rows at a time) on crafted positions whose groups span every row.

Columns of white stones from the top edge to the bottom edge between black walls, black to move: a white column with ONE empty end
is in atari (a black stone there captures all eighteen stones, rows 0 .. 17 or 1 .. 18), one with BOTH ends empty has two
liberties (a black stone on either end leaves it in atari: the group leaves M).  So nearly every first ply of every board
collects an eighteen- or seventeen-row group, including the odd last row pair of a 19-row board, and the games go on from the
captures.  Half the boards hold the transposed position (white rows: one row pair per group, nineteen columns).  The library is
sized for four compute units (GYMGO_AMD_CUS=4) so that 1 056 games take the kernel; every launch is checked against the pinned
C oracle.  Reference loop: gym_go/envs/go_env.py:49-81 over gym_go/gogame.py:34-87.
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

# column c %% 3 == 1 is white, the others black; white column k (k = 0 .. 5) leaves row 18 empty (k %% 3 == 0), row 0 (k %% 3 == 1)
# or both (k %% 3 == 2)
s0 = np.zeros((6, N, N), np.uint8)
for c in range(N):
    if c %% 3 != 1:
        s0[0, :, c] = 1
        continue
    k = c // 3
    s0[1, :, c] = 1
    if k %% 3 in (0, 2):
        s0[1, N - 1, c] = 0
    if k %% 3 in (1, 2):
        s0[1, 0, c] = 0
st_t = s0.transpose(0, 2, 1).copy()
B = 1056
states = np.stack([s0 if b %% 2 == 0 else st_t for b in range(B)])
for b in (0, 1):
    states[b, 3] = c_oracle.compute_invalid_moves(states[b], 1)   # (the mask of the player who moves after white: black)
states[0::2, 3] = states[0, 3]
states[1::2, 3] = states[1, 3]
legal = (states[0, 3] == 0) & (states[0, 0] == 0) & (states[0, 1] == 0)
assert int(legal.sum()) == 8, int(legal.sum())        # the eight empty column ends: every black stone plays next to a tall group
rng = gogame.rng_seed(B, 77, 0, 'cuda')
want, want_rng = states.copy(), rng.cpu().numpy().view(np.uint64).copy()
after1, _, last1 = c_oracle.batch_rollout_mt(states.copy(), want_rng.copy(), 1, True)
caught = (after1[:, 1].reshape(B, -1).sum(axis=1) < states[:, 1].reshape(B, -1).sum(axis=1))
assert int(caught.sum()) >= B // 4 and int((~caught).sum()) >= B // 8, int(caught.sum())   # captures and ataris both
for tracked in (False, True):
    st = torch.from_numpy(states).cuda()
    rng = gogame.rng_seed(B, 77, 0, 'cuda')
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
print('R5 OK')
''' % ROOT


def test_r5_collects_groups_that_span_every_row():
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    p = subprocess.run([sys.executable, '-c', SCRIPT], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'R5 OK' in p.stdout
