"""-m gpu: the `tactical` playout policy on the device, bit-exact against tests/mc_tactics_expect.py: the planes
(gogame.batch_tactics / batch_tactics_tracked, gymgo_amd/csrc/gg_tactics.h), batch_rollout_tracked(policy='tactical') on both
kernel families that carry the policy (k_rollout_lat_pol and k_rollout5_tac, gg_lat.h / gg_v5_kernel.h) and the Monte Carlo
stack above them.

The take-over tests size the library for FOUR compute units (GYMGO_AMD_CUS=4, read once per process: a process of its own, as
tests/test_gpu_playout_policy.py does), so that 19x19 batches above 512 games and 9x9 / 13x13 batches above 636 take k_rollout5_tac
for launches of >= 8 plies, batches up to 64 (19x19) / 256 games take k_rollout_lat_pol where the uniform path takes
k_rollout_lat, and the band in between - k_rollout4's for the uniform policy - takes k_rollout_lat_pol."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SIZES = tuple(range(2, 20))
SENTINEL = 0xA5


# ---------------------------------------------------------------- the planes
def _want_planes(states):
    import mc_tactics_expect as mt
    return np.stack(mt.tiers(states), axis=1).astype(np.uint8)


@pytest.mark.parametrize('N', SIZES)
def test_planes_byte_planes_and_tracked_every_size(N):
    import mc_tactics_expect as mt
    import plane_cases as pc
    from gymgo_amd import gogame
    states = np.concatenate([mt.pool(N), pc.states_of(N, 'clean')] + ([mt.seam_roots()] if N == 19 else []))
    B = len(states)
    want = _want_planes(states)
    assert not want[states[:, 5, 0, 0] != 0].any() and (states[:, 5, 0, 0] != 0).any()     # ended games: all zero
    if N >= 3:
        assert want[:, 0].any() and want[:, 1].any() and want[:, 2].any()
    st = torch.from_numpy(states).cuda()
    tr = gogame.batch_track(st)
    got = gogame.batch_tactics(st)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, 3, N, N)
    bad = np.flatnonzero((got.cpu().numpy() != want).reshape(B, -1).any(axis=1))
    assert len(bad) == 0, (N, bad[:8].tolist())
    assert torch.equal(gogame.batch_tactics_tracked(tr), got)                               # the two input forms, bit for bit
    # one dtype other than uint8, NumPy in and out, the single-state form
    h = gogame.batch_tactics(st, dtype=torch.float16)
    assert h.dtype == torch.float16 and torch.equal(h.to(torch.uint8), got)
    assert torch.equal(gogame.batch_tactics_tracked(tr, dtype=torch.float32).to(torch.uint8), got)
    assert np.array_equal(gogame.batch_tactics(states[:5]), want[:5])
    assert np.array_equal(gogame.tactics(states[1]), want[1])
    # one oriented call per form: row b is view orient[b] of its planes, and the planes of the turned position
    orient = ((np.arange(B) * 3 + 1) % 8).astype(np.int32)
    orient[0], orient[-1] = -3, 1 << 20 | 5
    o = torch.from_numpy(orient).cuda()
    turned = pc.turned(want, orient)
    for res in (gogame.batch_tactics(st, orient=o), gogame.batch_tactics_tracked(tr, orient=o)):
        assert np.array_equal(res.cpu().numpy(), turned), N
    assert np.array_equal(_want_planes(gogame.batch_symmetry(st, o & 7).cpu().numpy()), turned), N
    # out=: between sentinels, at an odd element offset
    raw = torch.full((B * 3 * N * N + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
    out = raw[7:7 + B * 3 * N * N].view(B, 3, N, N)
    assert gogame.batch_tactics(st, out=out) is out and torch.equal(out, got)
    assert bool((raw[:7] == SENTINEL).all()) and bool((raw[7 + B * 3 * N * N:] == SENTINEL).all())


def test_planes_on_the_hand_made_positions():
    import mc_tactics_expect as mt
    from gymgo_amd import gogame
    for name, b, C, E in mt.crafted_positions():
        got = gogame.tactics(b)
        assert got.dtype == np.uint8 and np.array_equal(got[0].astype(bool), C) and np.array_equal(got[1].astype(bool), E), name
        assert np.array_equal(got, _want_planes(b[None])[0]), name
    seam = mt.seam_roots()
    assert np.array_equal(gogame.batch_tactics(seam), _want_planes(seam))


TRIPS = r'''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
from gymgo_amd import gogame, _lib
import mc_tactics_expect as mt
assert _lib.lib().gg_device_cus() == 1
# 533 boards of 5x5 on ONE compute unit: 134 groups of four on a grid of 64 workgroups - workgroups 0 .. 5 make three trips of the
# grid-stride loop, the last group holds one board
N, B = 5, 533
p = mt.pool(N)
states = p[(5 * np.arange(B)) %% len(p)].copy()
want = np.stack(mt.tiers(states), axis=1).astype(np.uint8)
st = torch.from_numpy(states).cuda()
tr = gogame.batch_track(st)
for form, fn, x in (('bytes', gogame.batch_tactics, st), ('tracked', gogame.batch_tactics_tracked, tr)):
    for lead in (0, 3):
        raw = torch.full((B * 3 * N * N + 64,), 0xA5, dtype=torch.uint8, device='cuda')
        out = raw[lead:lead + B * 3 * N * N].view(B, 3, N, N)
        fn(x, out=out)
        bad = np.flatnonzero((out.cpu().numpy() != want).reshape(B, -1).any(axis=1))
        assert len(bad) == 0, (form, lead, bad[:8].tolist())
        assert bool((raw[:lead] == 0xA5).all()) and bool((raw[lead + B * 3 * N * N:] == 0xA5).all()), (form, lead)
    sub = fn(x[3:260])
    assert np.array_equal(sub.cpu().numpy(), want[3:260]), form
torch.cuda.synchronize()
print('TACTICS OK')
''' % (ROOT, os.path.join(ROOT, 'tests'))


# ---------------------------------------------------------------- the rollout in lockstep
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
import mc_tactics_expect as mt
import mc_puct_expect as pe
assert _lib.lib().gg_device_cus() == 4
LAUNCHES = (1, 2, 7, 8, 32)


def run(N, B, auto_reset, seed):
    """Boards, generators, last actions and step counts after every launch; and, on the restatement's trace, that the case
    drew from all three sets and saw a closed gate while a capture was there."""
    states = mt.rollout_batch(N, B)
    assert (states[:, 5, 0, 0] != 0).any() and (mp.candidates(states).sum(axis=1)[states[:, 5, 0, 0] == 0] == 0).any()
    st = torch.from_numpy(states).cuda()
    rng = gogame.rng_seed(B, seed, 0, 'cuda')
    want, want_rng = states.copy(), rng.cpu().numpy().view(np.uint64).copy()
    sd = torch.zeros(B, dtype=torch.int64, device='cuda')
    want_sd = np.zeros(B, np.int64)
    tr = gogame.batch_track(st)
    trace = []
    for F in LAUNCHES:
        la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
        gogame.batch_rollout_tracked(tr, rng, F, auto_reset, la, sd, policy='tactical')
        want, want_rng, want_last, steps = mt.tactical_rollout(want, want_rng, F, auto_reset, trace=trace)
        want_sd += steps
        got = gogame.batch_untrack(tr).cpu().numpy()
        bad = np.flatnonzero((got != want).reshape(B, -1).any(axis=1))
        assert len(bad) == 0, (N, B, F, auto_reset, bad[:6].tolist())
        assert np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng), (N, B, F, auto_reset)
        assert np.array_equal(la.cpu().numpy(), want_last), (N, B, F, auto_reset)
        assert np.array_equal(sd.cpu().numpy(), want_sd), (N, B, F, auto_reset)
    c = mt.trace_counts(trace)
    if N >= 3:
        assert c['C'] > 0 and c['E'] > 0 and c['F'] > 0 and c['closed_with_C'] > 0, (N, B, auto_reset, c)
    else:
        assert c['C'] > 0 and c['F'] > 0 and c['closed_with_C'] > 0, (N, B, auto_reset, c)
    return trace
''' % (ROOT, os.path.join(ROOT, 'tests'))

ROLLOUT_SIZES = PRELUDE + r'''
# every size at one small batch: k_rollout_lat_pol (k_rollout5_tac needs 513 / 637 games at four compute units)
for N in range(2, 20):
    for auto_reset in (False, True):
        run(N, 48, auto_reset, 300 + N)
print('TACTICS OK')
'''

ROLLOUT_19 = PRELUDE + r'''
# 4 CUs: up to 64 games k_rollout_lat_pol (where the uniform path takes k_rollout_lat), 65 .. 512 the band of k_rollout4 (here:
# k_rollout_lat_pol), from 513 games and 8 plies on k_rollout5_tac
for B in (33, 200, 513):
    for auto_reset in (False, True):
        trace = run(19, B, auto_reset, 100 + B)
        if B == 513:
            # the seam roots, 22 copies each: on the FIRST ply - the launch of one ply - some copy of either root has an open gate and
            # draws a capture across the pair's seam or on the board's edge
            live, before, n, act, which, gate, hasC = trace[0]
            # (the seam boards are the last 44 of the batch, all live: the last 44 rows of the ply's record)
            assert hasC[-44:].all() and (which[-44::2] == mt.SET_C).any() and (which[-43::2] == mt.SET_C).any()
print('TACTICS OK')
'''

ROLLOUT_SMALL = PRELUDE + r'''
# 9x9 / 13x13: k_rollout_lat_pol up to 256 games, k_rollout5_tac from 637 games and 8 plies on, the band in between
for N, sizes in ((9, (256, 300, 637)), (13, (255, 701))):
    for B in sizes:
        for auto_reset in (False, True):
            run(N, B, auto_reset, 200 + B + N)
print('TACTICS OK')
'''

STACK = PRELUDE + r'''
def cap(N):
    return -(-8 * N * N // 32) * 32   # max_plies: 8 N^2 rounded up to a multiple of every chunk length used here


def roots_of(N, R):
    p = mt.pool(N)
    return p[np.linspace(0, len(p) - 1, R).astype(int)]


# batch_playouts: ownership, komi, two slot counts (9x9: 640 slots - k_rollout5_tac - and 48 - k_rollout_lat_pol), two chunk lengths
for N, R, K in ((5, 12, 24), (9, 8, 80), (19, 8, 8)):
    roots = roots_of(N, R)
    dev = mc.to_dev(roots)
    want = mt.expected_playouts_tactical(roots, K, cap(N), komi=2.5, with_ownership=True)
    for slots, chunk in ((None, 32), (48, 8)):
        got = gogame.batch_playouts(dev, K, max_plies=cap(N), komi=2.5, ownership=True, slots=slots, chunk_plies=chunk,
                                    policy='tactical')
        mc.check(got, want, mc.KEYS + ('ownership',), (N, slots, chunk))
    a = gogame.batch_playouts(dev[:3], K, max_plies=cap(N), komi=2.5, policy='tactical')
    b = gogame.batch_playouts(dev[3:], K, max_plies=cap(N), komi=2.5, first_root=3, policy='tactical')
    for k in mc.KEYS:
        assert np.array_equal(np.concatenate([mc.to_np(getattr(a, k)), mc.to_np(getattr(b, k))]), want[k]), (N, k)
    one = gogame.playouts(roots[1], K, max_plies=cap(N), komi=2.5, first_root=1, policy='tactical')   # (root 1's jobs)
    assert int(one.black_wins) == int(want['black_wins'][1]) and int(one.plies_sum) == int(want['plies_sum'][1])
    assert bool((dev == mc.to_dev(roots)).all())

# batch_move_playouts and flat_mc_actions
for N, R, K in ((5, 6, 4), (9, 4, 2)):
    roots = roots_of(N, R)
    dev = mc.to_dev(roots)
    want = mt.expected_move_playouts_tactical(roots, K, cap(N), komi=0.5, first_root=2)
    for slots, chunk in ((None, 32), (40, 8)):
        got = gogame.batch_move_playouts(dev, K, max_plies=cap(N), komi=0.5, first_root=2, slots=slots, chunk_plies=chunk,
                                         policy='tactical')
        mc.check(got, want, ('legal',) + mc.KEYS, (N, slots, chunk))
    act = gogame.flat_mc_actions(dev, K, max_plies=cap(N), komi=0.5, first_root=2, policy='tactical')
    assert np.array_equal(mc.to_np(act), mc.flat_mc_choice(roots, want)), N

# batch_uct with its tree, and uct_actions
for N, R, I, K in ((5, 5, 10, 4), (9, 3, 6, 4)):
    roots = roots_of(N, R)
    dev = mc.to_dev(roots)
    want = mt.expected_uct_tactical(roots, I, K, max_plies=cap(N), komi=1.5, first_root=1)
    for slots, chunk in ((None, 32), (7, 16)):
        got = gogame.batch_uct(dev, I, K, max_plies=cap(N), komi=1.5, first_root=1, slots=slots, chunk_plies=chunk, tree=True, policy='tactical')
        mc.check(got, want, mc.ROOT_KEYS, (N, slots, chunk))
        mc.check(got.tree, want['tree'], mc.TREE_KEYS, (N, slots, chunk))
    act = gogame.uct_actions(dev, I, K, max_plies=cap(N), komi=1.5, first_root=1, policy='tactical')
    assert np.array_equal(mc.to_np(act), mc.most_visited(want)), N

# a PUCT search with playout_evaluator(policy='tactical') against the same search fed the expected values
N, I, K, f0 = 9, 16, 4, 2
roots = np.concatenate([mc.make_roots(N, 4, 5, max_ply=60, step=20)[1:], mc.crafted_roots(N)[1:]])
want = pe.expected_puct(roots, I, mt.playout_evaluator_np(K, 672, komi=0.5, seed=11, first_root=f0), komi=0.5)
ev = gogame.playout_evaluator(K, seed=11, first_root=f0, policy='tactical', slots=64, komi=0.5)
got = gogame.batch_puct(mc.to_dev(roots), I, ev, komi=0.5, tree=True)
pe.check(got, want, tag='tactical')
print('TACTICS OK')
'''

FORWARD = PRELUDE + r'''
# policies 0 and 1 through the _policy2 entry points equal the existing calls, tensor for tensor (on both sides of the take-over
# points); 'tactical' changes the games
stream = lambda: _lib.stream_ptr(torch.device('cuda', torch.cuda.current_device()))
for N, B in ((9, 300), (9, 700), (19, 40), (19, 600), (6, 90)):
    states = mt.rollout_batch(N, B)
    st = torch.from_numpy(states).cuda()
    results = {}
    for pol in (0, 1, 2):
        for name in ('gg_batch_rollout_tracked_policy', 'gg_batch_rollout_tracked_policy2'):
            if pol == 2 and not name.endswith('2'):
                continue
            tr, rng = gogame.batch_track(st), gogame.rng_seed(B, 5, 0, 'cuda')
            la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
            sd = torch.zeros(B, dtype=torch.int64, device='cuda')
            for F in (3, 9):
                _lib.call(name, tr, rng, la, sd, B, N, F, 0, pol, stream())
            results[(pol, name.endswith('2'))] = (tr, rng, la, sd)
    for pol in (0, 1):
        for x, y in zip(results[(pol, False)], results[(pol, True)]):
            assert torch.equal(x, y), (N, B, pol)
    assert not torch.equal(results[(1, True)][0], results[(2, True)][0]) and not torch.equal(results[(0, True)][0], results[(2, True)][0])
    t0, r0 = gogame.batch_track(st), gogame.rng_seed(B, 5, 0, 'cuda')
    gogame.batch_rollout_tracked(t0, r0, 3, False, policy='no_eye_fill')
    gogame.batch_rollout_tracked(t0, r0, 9, False, policy='no_eye_fill')
    assert torch.equal(t0, results[(1, True)][0]) and torch.equal(r0, results[(1, True)][1])
    try:
        _lib.call('gg_batch_rollout_tracked_policy', gogame.batch_track(st), gogame.rng_seed(B, 5, 0, 'cuda'), None, None, B, N, 3, 0, 2, stream())
        raise SystemExit('the _policy entry point took policy 2')
    except _lib.GymGoNativeError:
        pass

# the queue: batch_playouts / batch_move_playouts through gg_*_advance_policy2 with codes 0 and 1
import gymgo_amd.gogame as gg
N = 9
roots = mc.to_dev(mt.pool(N)[:10])
real = gg._run_queue


def through2(family, what, head, komi, bufs, counter, J, S, max_plies, chunk_plies, dev, policy=0):
    s = _lib.current_raw_stream(dev)
    _lib.call('gg_%s_begin' % family, *head, *bufs, s)
    gg._drive_playouts(lambda n: _lib.call('gg_%s_advance_policy2' % family, *head, float(komi), n, int(policy), *bufs, s),
                       counter, J, S, max_plies, chunk_plies, dev, what)


for policy in ('uniform', 'no_eye_fill'):
    a = gogame.batch_playouts(roots, 8, komi=0.5, ownership=True, policy=policy)
    m = gogame.batch_move_playouts(roots[:3], 2, komi=0.5, policy=policy)
    gg._run_queue = through2
    try:
        b = gogame.batch_playouts(roots, 8, komi=0.5, ownership=True, policy=policy)
        n = gogame.batch_move_playouts(roots[:3], 2, komi=0.5, policy=policy)
    finally:
        gg._run_queue = real
    for x, y in list(zip(a, b)) + list(zip(m, n)):
        assert torch.equal(x, y), policy
t = gogame.batch_playouts(roots, 8, komi=0.5, policy='tactical')
assert not torch.equal(t.plies_sum, gogame.batch_playouts(roots, 8, komi=0.5, policy='no_eye_fill').plies_sum)
print('TACTICS OK')
'''


def _run(script, cus='4'):
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = cus
    p = subprocess.run([sys.executable, '-c', script], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'TACTICS OK' in p.stdout


def test_planes_on_later_trips_of_the_grid_stride_loop():
    _run(TRIPS, cus='1')


def test_tactical_rollout_every_size_in_lockstep():
    _run(ROLLOUT_SIZES)


def test_tactical_rollout_19x19_both_families_and_the_band():
    _run(ROLLOUT_19)


def test_tactical_rollout_small_boards_both_families_and_the_band():
    _run(ROLLOUT_SMALL)


def test_tactical_playouts_move_playouts_uct_and_puct_against_their_expectations():
    _run(STACK)


def test_policies_0_and_1_through_policy2_equal_the_existing_calls_and_tactical_changes_the_games():
    _run(FORWARD)
