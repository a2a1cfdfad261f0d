"""-m gpu: the `no_eye_fill` playout policy on the device, bit-exact against tests/mc_policy_expect.py: gogame.batch_eye_mask,
batch_rollout_tracked(policy=...) on both kernel families that carry the policy (k_rollout_lat's plain tracked form and
k_rollout5, gymgo_amd/csrc/gg_lat.h / gg_v5_kernel.h) and the Monte Carlo stack above them.

The take-over tests size the library for FOUR compute units (GYMGO_AMD_CUS=4, read once per process: a process of its own, as
tests/test_gpu_r5.py does), so that 19x19 batches above 512 games and 9x9 / 13x13 batches above 636 take k_rollout5 for
launches of >= 8 plies, batches up to 64 (19x19) / 256 games take k_rollout_lat where the uniform path does, and the band in
between - k_rollout4's for the uniform policy - takes k_rollout_lat."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = r'''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
from gymgo_amd import gogame, _lib
from oracle import c_oracle
import mc_expect as mc
import mc_policy_expect as mp
assert _lib.lib().gg_device_cus() == 4


def pool(N):
    """Roots of every kind: random positions (the last one a finished game), the empty board, a root after a pass, a ko root,
    a finished game, roots whose mover has no candidate, and at 19x19 eyes on the seam rows of a k_rollout5 pair."""
    parts = [mc.make_roots(N, 24, 5 + N, max_ply=2 * N * N, step=max(2, N * N // 12)), mc.crafted_roots(N), mp.forced_pass_roots(N)]
    if N == 19:
        parts.append(mp.seam_roots())
    return np.concatenate(parts)


def run(N, B, launches, auto_reset, seed):
    roots = pool(N)
    states = roots[np.arange(B) %% len(roots)].copy()
    st = torch.from_numpy(states).cuda()
    rng = gogame.rng_seed(B, seed, 0, 'cuda')
    want, want_rng = states.copy(), rng.cpu().numpy().view(np.uint64).copy()
    sd = torch.zeros(B, dtype=torch.int64, device='cuda')
    want_sd = np.zeros(B, np.int64)
    tr = gogame.batch_track(st)
    for F in launches:
        la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
        gogame.batch_rollout_tracked(tr, rng, F, auto_reset, la, sd, policy='no_eye_fill')
        want, want_rng, want_last, steps = mp.policy_rollout(want, want_rng, F, auto_reset)
        want_sd += steps
        got = gogame.batch_untrack(tr).cpu().numpy()
        bad = np.flatnonzero((got != want).reshape(B, -1).any(axis=1))
        assert len(bad) == 0, (N, B, F, auto_reset, bad[:6].tolist())
        assert np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng), (N, B, F, auto_reset)
        assert np.array_equal(la.cpu().numpy(), want_last), (N, B, F, auto_reset)
        assert np.array_equal(sd.cpu().numpy(), want_sd), (N, B, F, auto_reset)
''' % (ROOT, os.path.join(ROOT, 'tests'))

LAUNCHES = (1, 2, 7, 8, 32, 256)

ROLLOUT_19 = PRELUDE + r'''
# 4 CUs: up to 64 games k_rollout_lat (as the uniform path), 65 .. 512 the band of k_rollout4 (here: k_rollout_lat), from 513 games
# and 8 plies on k_rollout5
for B in (33, 64, 200, 512, 513, 600):
    for auto_reset in (False, True):
        run(19, B, %r, auto_reset, 100 + B)
print('POLICY OK')
''' % (LAUNCHES,)

ROLLOUT_SMALL = PRELUDE + r'''
# 9x9 / 13x13: k_rollout_lat up to 256 games, k_rollout5 from 637 games and 8 plies on, the band in between; every other size: k_rollout_lat
for N, sizes in ((9, (256, 300, 636, 637, 700)), (13, (255, 640, 701)), (5, (37, 700)), (7, (130, 641))):
    for B in sizes:
        for auto_reset in (False, True):
            run(N, B, %r, auto_reset, 200 + B + N)
print('POLICY OK')
''' % (LAUNCHES,)

STACK = PRELUDE + r'''
def cap(N):
    return -(-8 * N * N // 32) * 32   # max_plies: 8 N^2 rounded up to a multiple of every chunk length used here


def roots_of(N, R):
    p = pool(N)
    return p[np.linspace(0, len(p) - 1, R).astype(int)]


# batch_playouts: ownership, komi, first_root shards, two slot counts (19x19: 1 024 slots - k_rollout5 - and 48 - k_rollout_lat),
# two chunk lengths
for N, R, K in ((5, 12, 40), (9, 10, 32), (19, 8, 136)):
    roots = roots_of(N, R)
    dev = mc.to_dev(roots)
    want = mp.expected_playouts_policy(roots, K, cap(N), komi=2.5, with_ownership=True)
    for slots, chunk in ((None, 32), (48, 8), (None, 8)):
        got = gogame.batch_playouts(dev, K, max_plies=cap(N), komi=2.5, ownership=True, slots=slots, chunk_plies=chunk,
                                    policy='no_eye_fill')
        mc.check(got, want, mc.KEYS + ('ownership',), (N, slots, chunk))
    a = gogame.batch_playouts(dev[:3], K, max_plies=cap(N), komi=2.5, policy='no_eye_fill')
    b = gogame.batch_playouts(dev[3:], K, max_plies=cap(N), komi=2.5, first_root=3, policy='no_eye_fill')
    for k in mc.KEYS:
        assert np.array_equal(np.concatenate([mc.to_np(getattr(a, k)), mc.to_np(getattr(b, k))]), want[k]), (N, k)

# batch_move_playouts and flat_mc_actions
for N, R, K in ((5, 8, 6), (9, 5, 3), (19, 3, 1)):
    roots = roots_of(N, R)
    dev = mc.to_dev(roots)
    want = mp.expected_move_playouts_policy(roots, K, cap(N), komi=0.5, first_root=2)
    for slots, chunk in ((None, 32), (40, 8)):
        got = gogame.batch_move_playouts(dev, K, max_plies=cap(N), komi=0.5, first_root=2, slots=slots, chunk_plies=chunk,
                                         policy='no_eye_fill')
        mc.check(got, want, ('legal',) + mc.KEYS, (N, slots, chunk))
    act = gogame.flat_mc_actions(dev, K, max_plies=cap(N), komi=0.5, first_root=2, policy='no_eye_fill')
    assert np.array_equal(mc.to_np(act), mc.flat_mc_choice(roots, want)), N

# batch_uct and uct_actions
for N, R, I, K in ((5, 6, 12, 4), (9, 4, 6, 4), (19, 3, 3, 2)):
    roots = roots_of(N, R)
    dev = mc.to_dev(roots)
    want = mp.expected_uct_policy(roots, I, K, max_plies=cap(N), komi=1.5, first_root=1)
    for slots, chunk in ((None, 32), (7, 16)):
        got = gogame.batch_uct(dev, I, K, max_plies=cap(N), komi=1.5, first_root=1, slots=slots, chunk_plies=chunk, tree=True, policy='no_eye_fill')
        mc.check(got, want, mc.ROOT_KEYS, (N, slots, chunk))
        mc.check(got.tree, want['tree'], mc.TREE_KEYS, (N, slots, chunk))
    act = gogame.uct_actions(dev, I, K, max_plies=cap(N), komi=1.5, first_root=1, policy='no_eye_fill')
    assert np.array_equal(mc.to_np(act), mc.most_visited(want)), N
print('POLICY OK')
'''


def _run(script):
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    p = subprocess.run([sys.executable, '-c', script], env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'POLICY OK' in p.stdout


def test_policy_rollout_19x19_both_families_and_the_band():
    _run(ROLLOUT_19)


def test_policy_rollout_small_boards_both_families_and_the_band():
    _run(ROLLOUT_SMALL)


def test_policy_playouts_move_playouts_and_uct_against_their_expectations():
    _run(STACK)


def test_eye_mask_on_crafted_and_random_positions():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import mc_expect as mc
    import mc_policy_expect as mp
    from gymgo_amd import gogame
    boards, want = mp.crafted_eye_boards()
    for b, w in zip(boards, want):
        got = gogame.eye_mask(b)
        assert got.dtype == np.uint8 and np.array_equal(got.astype(bool), w)
        assert np.array_equal(gogame.batch_eye_mask(torch.from_numpy(b[None]).cuda()).cpu().numpy()[0].astype(bool), w)
    some = 0
    for N in (5, 9, 13, 19):
        roots = np.concatenate([mc.make_roots(N, 64, 3 + N, max_ply=3 * N * N, step=max(2, N * N // 16)), mc.crafted_roots(N),
                                mp.forced_pass_roots(N)] + ([mp.seam_roots()] if N == 19 else []))
        want = mp.eyes(roots)
        got = gogame.batch_eye_mask(roots)
        assert got.shape == (len(roots), N, N) and np.array_equal(got.astype(bool), want), N
        assert not got[roots[:, 5, 0, 0] != 0].any()
        some += int(want.sum())
    assert some > 20


def test_uniform_policy_is_the_call_without_the_keyword():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import mc_expect as mc
    from gymgo_amd import gogame
    N = 9
    roots = mc.make_roots(N, 6, 4, max_ply=60, step=10)
    dev = mc.to_dev(roots)
    a = gogame.batch_playouts(dev, 16, komi=0.5, ownership=True)
    b = gogame.batch_playouts(dev, 16, komi=0.5, ownership=True, policy='uniform')
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    a = gogame.batch_move_playouts(dev[:2], 2)
    b = gogame.batch_move_playouts(dev[:2], 2, policy='uniform')
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    a = gogame.batch_uct(dev[:3], 4, 4)
    b = gogame.batch_uct(dev[:3], 4, 4, policy='uniform')
    for x, y in zip(a[:-1], b[:-1]):
        assert torch.equal(x, y)
    assert torch.equal(gogame.flat_mc_actions(dev[:2], 2), gogame.flat_mc_actions(dev[:2], 2, policy='uniform'))
    assert torch.equal(gogame.uct_actions(dev[:3], 4, 4), gogame.uct_actions(dev[:3], 4, 4, policy='uniform'))
    B = 300
    st = gogame.batch_init_state(B, N, device='cuda')
    tr, tr2 = gogame.batch_track(st), gogame.batch_track(st)
    r1, r2 = gogame.rng_seed(B, 5, 0, 'cuda'), gogame.rng_seed(B, 5, 0, 'cuda')
    gogame.batch_rollout_tracked(tr, r1, 40, False)
    gogame.batch_rollout_tracked(tr2, r2, 40, False, policy='uniform')
    assert torch.equal(tr, tr2) and torch.equal(r1, r2)
    # ... and the policy changes the games
    tr3, r3 = gogame.batch_track(st), gogame.rng_seed(B, 5, 0, 'cuda')
    gogame.batch_rollout_tracked(tr3, r3, 40, False, policy='no_eye_fill')
    assert not torch.equal(tr, tr3)
