"""-m gpu: the `pattern` playout policy on the device, bit-exact against tests/mc_pattern_expect.py: the planes
(gogame.batch_patterns / batch_patterns_tracked, gymgo_amd/csrc/gg_pattern.h), batch_rollout_tracked(policy='pattern') with
last_actions carried from launch to launch on both kernel families that carry the policy (k_rollout_lat_pol and k_rollout5_pat,
gg_lat.h / gg_v5_kernel.h) and the Monte Carlo stack above them.

The take-over tests size the library for FOUR compute units (GYMGO_AMD_CUS=4, read once per process: a process of its own, as
tests/test_gpu_tactics.py does), so that 19x19 batches above 512 games and 9x9 / 13x13 batches above 636 take k_rollout5_pat for
launches of >= 8 plies and everything else k_rollout_lat_pol.  tests/test_pattern_host.py asserts the premises of these cases on
the CPU: their traces draw from L, see an open gate with C and E empty and L not, and a previous pass; L crosses the 19x19 seam."""
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


def _stream():
    from gymgo_amd import _lib
    return _lib.stream_ptr(torch.device('cuda', torch.cuda.current_device()))


# ---------------------------------------------------------------- the planes
def _want_planes(states, last):
    import mc_pattern_expect as mq
    return np.stack(mq.pattern_sets(states, last), axis=1).astype(np.uint8)


def _all_boards(N):
    """Every board of N x N with arbitrary stones (3^(N^2) of them), a zero invalid plane, the turn by the board's number, and
    previous actions that cycle over every point, the pass and -1 - every neighbourhood that can occur, off-board ones included."""
    P = N * N
    n = 3 ** P
    digits = (np.arange(n)[:, None] // 3 ** np.arange(P)[None, :]) % 3
    states = np.zeros((n, 6, N, N), np.uint8)
    states[:, 0] = (digits == 1).reshape(n, N, N)
    states[:, 1] = (digits == 2).reshape(n, N, N)
    states[:, 2] = ((np.arange(n) // 7) % 2).astype(np.uint8)[:, None, None]
    last = ((np.arange(n) * 5) % (P + 2) - 1).astype(np.int32)
    return states, last


@pytest.mark.parametrize('N', (3, 2))
def test_planes_on_every_board_of_a_small_size(N):
    from gymgo_amd import gogame
    states, last = _all_boards(N)
    want = _want_planes(states, last)
    assert want[:, 0].any() and want[:, 1].any()
    st = torch.from_numpy(states).cuda()
    got = gogame.batch_patterns(st, torch.from_numpy(last).cuda())
    bad = np.flatnonzero((got.cpu().numpy() != want).reshape(len(states), -1).any(axis=1))
    assert len(bad) == 0, (N, bad[:8].tolist())
    assert not gogame.batch_patterns(st)[:, 1].any()                                        # no last: L is empty
    assert torch.equal(gogame.batch_patterns(st)[:, 0], got[:, 0])


@pytest.mark.parametrize('N', SIZES)
def test_planes_byte_planes_and_tracked_every_size(N):
    import mc_pattern_expect as mq
    import mc_tactics_expect as mt
    import plane_cases as pc
    from gymgo_amd import gogame
    parts = [mt.pool(N), pc.states_of(N, 'clean')] + ([mq.seam_roots()[0]] if N == 19 else [])
    states = np.concatenate(parts)
    B = len(states)
    last = mq.last_cycle(N, B)
    if N == 19:
        last[-len(parts[-1]):] = mq.seam_roots()[1]
    want = _want_planes(states, last)
    assert not want[states[:, 5, 0, 0] != 0].any() and (states[:, 5, 0, 0] != 0).any()     # ended games: all zero
    assert want[:, 0].any() and (want[:, 1].any() or N == 2)
    st = torch.from_numpy(states).cuda()
    la = torch.from_numpy(last).cuda()
    tr = gogame.batch_track(st)
    got = gogame.batch_patterns(st, la)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, 2, N, N)
    bad = np.flatnonzero((got.cpu().numpy() != want).reshape(B, -1).any(axis=1))
    assert len(bad) == 0, (N, bad[:8].tolist())
    assert torch.equal(gogame.batch_patterns_tracked(tr, la), got)                          # the two input forms, bit for bit
    assert torch.equal(la, torch.from_numpy(last).cuda())                                   # last is an input
    # one dtype other than uint8, NumPy in and out, the single-state form
    h = gogame.batch_patterns(st, la, dtype=torch.float16)
    assert h.dtype == torch.float16 and torch.equal(h.to(torch.uint8), got)
    assert np.array_equal(gogame.batch_patterns(states[:5], last[:5]), want[:5])
    i = int(np.flatnonzero(want[:, 1].reshape(B, -1).any(axis=1))[0]) if want[:, 1].any() else 1
    assert np.array_equal(gogame.patterns(states[i], int(last[i])), want[i])
    # one oriented call per form: row b is view orient[b] of its planes - last refers to the unturned board
    orient = ((np.arange(B) * 3 + 1) % 8).astype(np.int32)
    orient[0], orient[-1] = -3, 1 << 20 | 5
    o = torch.from_numpy(orient).cuda()
    turned = pc.turned(want, orient)
    for res in (gogame.batch_patterns(st, la, orient=o), gogame.batch_patterns_tracked(tr, la, orient=o)):
        assert np.array_equal(res.cpu().numpy(), turned), N
    # out=: between sentinels, at an odd element offset
    raw = torch.full((B * 2 * N * N + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
    out = raw[7:7 + B * 2 * N * N].view(B, 2, N, N)
    assert gogame.batch_patterns(st, la, out=out) is out and torch.equal(out, got)
    assert bool((raw[:7] == SENTINEL).all()) and bool((raw[7 + B * 2 * N * N:] == SENTINEL).all())


def test_planes_on_the_hand_made_positions():
    import mc_pattern_expect as mq
    from gymgo_amd import gogame
    for name, b, prev, P, L in mq.crafted_positions():
        N = b.shape[-1]
        got = gogame.patterns(b, None if prev is None else prev[0] * N + prev[1])
        assert got.dtype == np.uint8 and np.array_equal(got[0].astype(bool), P) and np.array_equal(got[1].astype(bool), L), name


TRIPS = r'''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
from gymgo_amd import gogame, _lib
import mc_tactics_expect as mt
import mc_pattern_expect as mq
assert _lib.lib().gg_device_cus() == 1
# 533 boards of 5x5 on ONE compute unit: 134 groups of four on a grid of 64 workgroups - workgroups 0 .. 5 make three trips of the
# grid-stride loop, the last group holds one board
N, B = 5, 533
p = mt.pool(N)
states = p[(5 * np.arange(B)) %% len(p)].copy()
last = mq.last_cycle(N, B)
want = np.stack(mq.pattern_sets(states, last), axis=1).astype(np.uint8)
st = torch.from_numpy(states).cuda()
la = torch.from_numpy(last).cuda()
tr = gogame.batch_track(st)
for form, fn, x in (('bytes', gogame.batch_patterns, st), ('tracked', gogame.batch_patterns_tracked, tr)):
    for lead in (0, 3):
        raw = torch.full((B * 2 * N * N + 64,), 0xA5, dtype=torch.uint8, device='cuda')
        out = raw[lead:lead + B * 2 * N * N].view(B, 2, N, N)
        fn(x, la, out=out)
        bad = np.flatnonzero((out.cpu().numpy() != want).reshape(B, -1).any(axis=1))
        assert len(bad) == 0, (form, lead, bad[:8].tolist())
        assert bool((raw[:lead] == 0xA5).all()) and bool((raw[lead + B * 2 * N * N:] == 0xA5).all()), (form, lead)
    sub = fn(x[3:260], la[3:260])
    assert np.array_equal(sub.cpu().numpy(), want[3:260]), form
torch.cuda.synchronize()
print('PATTERN OK')
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
import mc_pattern_expect as mq
import mc_puct_expect as pe
assert _lib.lib().gg_device_cus() == 4
LAUNCHES = (1, 2, 7, 8, 32)


def run(N, B, auto_reset, seed):
    """Boards, generators, last actions and step counts after every launch, last_actions carried from launch to launch; then the
    same total in ONE launch from the same start gives the same boards and generators."""
    states, last0 = mq.rollout_batch(N, B)
    st = torch.from_numpy(states).cuda()
    rng = gogame.rng_seed(B, seed, 0, 'cuda')
    rng0 = rng.clone()
    want, want_rng = states.copy(), rng.cpu().numpy().view(np.uint64).copy()
    sd = torch.zeros(B, dtype=torch.int64, device='cuda')
    want_sd = np.zeros(B, np.int64)
    tr = gogame.batch_track(st)
    la = torch.from_numpy(last0).cuda()
    want_last = last0
    trace = []
    for F in LAUNCHES:
        gogame.batch_rollout_tracked(tr, rng, F, auto_reset, la, sd, policy='pattern')
        want, want_rng, want_last, steps = mq.pattern_rollout(want, want_rng, F, auto_reset, last=want_last, trace=trace)
        want_sd += steps
        got = gogame.batch_untrack(tr).cpu().numpy()
        bad = np.flatnonzero((got != want).reshape(B, -1).any(axis=1))
        assert len(bad) == 0, (N, B, F, auto_reset, bad[:6].tolist())
        assert np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng), (N, B, F, auto_reset)
        assert np.array_equal(la.cpu().numpy(), want_last), (N, B, F, auto_reset)
        assert np.array_equal(sd.cpu().numpy(), want_sd), (N, B, F, auto_reset)
    tr1, la1 = gogame.batch_track(st), torch.from_numpy(last0).cuda()
    gogame.batch_rollout_tracked(tr1, rng0, sum(LAUNCHES), auto_reset, la1, policy='pattern')
    assert torch.equal(tr1, tr) and torch.equal(rng0, rng), (N, B, auto_reset, 'one launch')
    c = mq.trace_counts(trace)
    if N >= 3:
        assert c['L'] > 0 and c['open_L_only'] > 0 and c['after_pass'] > 0, (N, B, auto_reset, c)
    return trace
''' % (ROOT, os.path.join(ROOT, 'tests'))

ROLLOUT_SIZES = PRELUDE + r'''
# every size at one small batch: k_rollout_lat_pol (k_rollout5_pat needs 513 / 637 games at four compute units)
for N in range(%d, %d):
    for auto_reset in (False, True):
        run(N, 48, auto_reset, 300 + N)
# None for last_actions: no board has a previous point - what a tensor of -1 gives
st, _ = mq.rollout_batch(7, 40)
a, b = gogame.batch_track(torch.from_numpy(st).cuda()), gogame.batch_track(torch.from_numpy(st).cuda())
ra, rb = gogame.rng_seed(40, 3, 0, 'cuda'), gogame.rng_seed(40, 3, 0, 'cuda')
gogame.batch_rollout_tracked(a, ra, 9, False, None, policy='pattern')
gogame.batch_rollout_tracked(b, rb, 9, False, torch.full((40,), -1, dtype=torch.int32, device='cuda'), policy='pattern')
assert torch.equal(a, b) and torch.equal(ra, rb)
print('PATTERN OK')
'''

ROLLOUT_19 = PRELUDE + r'''
# 4 CUs: up to 512 games k_rollout_lat_pol (the uniform path's k_rollout_lat and the band of k_rollout4), from 513 games and 8
# plies on k_rollout5_pat.  The last 48 boards are the seam roots with their previous moves in rows 9 / 10, 0 / 18, columns 0 / 18
# and the corners: on the first ply - the launch of one ply - some copies have an open gate and answer locally
for B in (@B@,):
    for auto_reset in (@AUTO@,):
        trace = run(19, B, auto_reset, 100 + B)
        live, before, n, act, which, gate, onlyL, prev, Lp = trace[0]
        k = min(48, B // 2)
        assert (which[-k:] == mq.SET_L).any()
print('PATTERN OK')
'''

ROLLOUT_SMALL = PRELUDE + r'''
# 9x9 / 13x13: k_rollout_lat_pol up to 636 games, k_rollout5_pat from 637 games and 8 plies on
for N, sizes in ((@N@, @SIZES@),):
    for B in sizes:
        for auto_reset in (False, True):
            run(N, B, auto_reset, 200 + B + N)
print('PATTERN OK')
'''

STACK_HELPERS = r'''
def cap(N):
    return -(-8 * N * N // 64) * 64   # max_plies: 8 N^2 rounded up to a multiple of every chunk length used here


def roots_of(N, R):
    p = mt.pool(N)
    return p[np.linspace(0, len(p) - 1, R).astype(int)]


'''

STACK_PLAYOUTS = PRELUDE + STACK_HELPERS + r'''
# batch_playouts: ownership, komi, slot counts on both kernel families (9x9: 640 slots - k_rollout5_pat - and fewer -
# k_rollout_lat_pol) x chunk lengths 8, 32, 64: identical results; shards by first_root concatenate
for N, R, K in (@CASE@,):
    roots = roots_of(N, R)
    dev = mc.to_dev(roots)
    want = mq.expected_playouts_pattern(roots, K, cap(N), komi=2.5, with_ownership=True)
    for slots, chunk in ((None, 32), (48, 8), (7, 64), (640, 8), (33, 32)):
        got = gogame.batch_playouts(dev, K, max_plies=cap(N), komi=2.5, ownership=True, slots=slots, chunk_plies=chunk,
                                    policy='pattern')
        mc.check(got, want, mc.KEYS + ('ownership',), (N, slots, chunk))
    a = gogame.batch_playouts(dev[:3], K, max_plies=cap(N), komi=2.5, policy='pattern')
    b = gogame.batch_playouts(dev[3:], K, max_plies=cap(N), komi=2.5, first_root=3, policy='pattern')
    for k in mc.KEYS:
        assert np.array_equal(np.concatenate([mc.to_np(getattr(a, k)), mc.to_np(getattr(b, k))]), want[k]), (N, k)
    one = gogame.playouts(roots[1], K, max_plies=cap(N), komi=2.5, first_root=1, policy='pattern')   # (root 1's jobs)
    assert int(one.black_wins) == int(want['black_wins'][1]) and int(one.plies_sum) == int(want['plies_sum'][1])
    assert bool((dev == mc.to_dev(roots)).all())
    t = gogame.batch_playouts(dev, K, max_plies=cap(N), komi=2.5, policy='tactical')
    assert not torch.equal(t.plies_sum, got.plies_sum), N                                            # not the tactical playouts

print('PATTERN OK')
'''

STACK_MOVES = PRELUDE + STACK_HELPERS + r'''
# batch_move_playouts and flat_mc_actions
for N, R, K in (@CASE@,):
    roots = roots_of(N, R)
    dev = mc.to_dev(roots)
    want = mq.expected_move_playouts_pattern(roots, K, cap(N), komi=0.5, first_root=2)
    for slots, chunk in ((None, 32), (40, 8), (9, 64)):
        got = gogame.batch_move_playouts(dev, K, max_plies=cap(N), komi=0.5, first_root=2, slots=slots, chunk_plies=chunk,
                                         policy='pattern')
        mc.check(got, want, ('legal',) + mc.KEYS, (N, slots, chunk))
    act = gogame.flat_mc_actions(dev, K, max_plies=cap(N), komi=0.5, first_root=2, policy='pattern')
    assert np.array_equal(mc.to_np(act), mc.flat_mc_choice(roots, want)), N

print('PATTERN OK')
'''

STACK_UCT = PRELUDE + STACK_HELPERS + r'''
# batch_uct with its whole tree, and uct_actions
for N, R, I, K in (@CASE@,):
    roots = roots_of(N, R)
    dev = mc.to_dev(roots)
    want = mq.expected_uct_pattern(roots, I, K, max_plies=cap(N), komi=1.5, first_root=1)
    for slots, chunk in ((None, 32), (7, 16)):
        got = gogame.batch_uct(dev, I, K, max_plies=cap(N), komi=1.5, first_root=1, slots=slots, chunk_plies=chunk, tree=True, policy='pattern')
        mc.check(got, want, mc.ROOT_KEYS, (N, slots, chunk))
        mc.check(got.tree, want['tree'], mc.TREE_KEYS, (N, slots, chunk))
    act = gogame.uct_actions(dev, I, K, max_plies=cap(N), komi=1.5, first_root=1, policy='pattern')
    assert np.array_equal(mc.to_np(act), mc.most_visited(want)), N

print('PATTERN OK')
'''

STACK_PUCT = PRELUDE + r'''
# a PUCT search with playout_evaluator(policy='pattern') against the same search fed the expected values
N, I, K, f0 = 9, 16, 4, 2
roots = np.concatenate([mc.make_roots(N, 4, 5, max_ply=60, step=20)[1:], mc.crafted_roots(N)[1:]])
want = pe.expected_puct(roots, I, mq.playout_evaluator_np(K, 672, komi=0.5, seed=11, first_root=f0), komi=0.5)
ev = gogame.playout_evaluator(K, seed=11, first_root=f0, policy='pattern', slots=64, komi=0.5)
got = gogame.batch_puct(mc.to_dev(roots), I, ev, komi=0.5, tree=True)
pe.check(got, want, tag='pattern')
print('PATTERN OK')
'''

FORWARD = PRELUDE + r'''
# policies 0, 1 and 2 through the _policy3 entry points equal the _policy2 calls, tensor for tensor (on both sides of the
# take-over points), and leave last untouched where it is only an output of the rollout's last action; 'pattern' changes the games
stream = lambda: _lib.stream_ptr(torch.device('cuda', torch.cuda.current_device()))
for N, B in ((9, 300), (9, 700), (19, 40), (19, 600), (6, 90)):
    states, last0 = mq.rollout_batch(N, B)
    st = torch.from_numpy(states).cuda()
    results = {}
    for pol in (0, 1, 2, 3):
        for name in ('gg_batch_rollout_tracked_policy2', 'gg_batch_rollout_tracked_policy3'):
            if pol == 3 and not name.endswith('3'):
                continue
            tr, rng = gogame.batch_track(st), gogame.rng_seed(B, 5, 0, 'cuda')
            la = torch.from_numpy(last0).cuda()
            sd = torch.zeros(B, dtype=torch.int64, device='cuda')
            for F in (3, 9):
                _lib.call(name, tr, rng, la, sd, B, N, F, 0, pol, stream())
            results[(pol, name.endswith('3'))] = (tr, rng, la, sd)
            if pol < 3:      # ... and with no last_actions at all
                tr2, rng2 = gogame.batch_track(st), gogame.rng_seed(B, 5, 0, 'cuda')
                for F in (3, 9):
                    _lib.call(name, tr2, rng2, None, None, B, N, F, 0, pol, stream())
                assert torch.equal(tr2, tr) and torch.equal(rng2, rng), (N, B, pol, name)
    for pol in (0, 1, 2):
        for x, y in zip(results[(pol, False)], results[(pol, True)]):
            assert torch.equal(x, y), (N, B, pol)
    assert not torch.equal(results[(2, True)][0], results[(3, True)][0]) and not torch.equal(results[(1, True)][0], results[(3, True)][0])
    for name in ('gg_batch_rollout_tracked_policy', 'gg_batch_rollout_tracked_policy2'):
        try:
            _lib.call(name, gogame.batch_track(st), gogame.rng_seed(B, 5, 0, 'cuda'), None, None, B, N, 3, 0, 3, stream())
            raise SystemExit(name + ' took policy 3')
        except _lib.GymGoNativeError:
            pass
    try:     # policy 3 without last_actions
        _lib.call('gg_batch_rollout_tracked_policy3', gogame.batch_track(st), gogame.rng_seed(B, 5, 0, 'cuda'), None, None, B, N, 3, 0, 3, stream())
        raise SystemExit('policy 3 ran without last_actions')
    except _lib.GymGoNativeError:
        pass

# the queue: batch_playouts / batch_move_playouts through gg_*_advance_policy3 with codes 0, 1 and 2 - last NULL, and a last that
# must stay as it is
import gymgo_amd.gogame as gg
N = 9
roots = mc.to_dev(mt.pool(N)[:10])
real = gg._run_queue
canary = [None]


def through3(family, what, head, komi, bufs, counter, J, S, max_plies, chunk_plies, dev, policy=0):
    s = _lib.current_raw_stream(dev)
    _lib.call('gg_%s_begin' % family, *head, *bufs, s)
    gg._drive_playouts(lambda n: _lib.call('gg_%s_advance_policy3' % family, *head, float(komi), n, int(policy), *bufs, canary[0], s),
                       counter, J, S, max_plies, chunk_plies, dev, what)


for policy in ('uniform', 'no_eye_fill', 'tactical'):
    a = gogame.batch_playouts(roots, 8, komi=0.5, ownership=True, policy=policy, slots=64)
    m = gogame.batch_move_playouts(roots[:3], 2, komi=0.5, policy=policy, slots=64)
    for c in (None, torch.full((64,), 77, dtype=torch.int32, device='cuda')):
        canary[0] = c
        gg._run_queue = through3
        try:
            b = gogame.batch_playouts(roots, 8, komi=0.5, ownership=True, policy=policy, slots=64)
            n = gogame.batch_move_playouts(roots[:3], 2, komi=0.5, policy=policy, slots=64)
        finally:
            gg._run_queue = real
        for x, y in list(zip(a, b)) + list(zip(m, n)):
            assert torch.equal(x, y), policy
        assert c is None or bool((c == 77).all()), policy
print('PATTERN OK')
'''


def _run(script, cus='4'):
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = cus
    p = subprocess.run([sys.executable, '-c', script], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'PATTERN OK' in p.stdout


def test_planes_on_later_trips_of_the_grid_stride_loop():
    _run(TRIPS, cus='1')


@pytest.mark.parametrize('lo', (2, 5, 8, 11, 14, 17))
def test_pattern_rollout_every_size_in_lockstep(lo):
    _run(ROLLOUT_SIZES % (lo, lo + 3))


@pytest.mark.parametrize('auto_reset', (False, True))
@pytest.mark.parametrize('B', (33, 200, 513))
def test_pattern_rollout_19x19_both_families_and_the_band(B, auto_reset):
    _run(ROLLOUT_19.replace('@B@', str(B)).replace('@AUTO@', str(auto_reset)))


@pytest.mark.parametrize('N, sizes', ((9, (256, 300)), (9, (637,)), (13, (255,)), (13, (701,))))
def test_pattern_rollout_small_boards_both_families_and_the_band(N, sizes):
    _run(ROLLOUT_SMALL.replace('@N@', str(N)).replace('@SIZES@', repr(sizes)))


@pytest.mark.parametrize('case', ((5, 12, 24), (9, 8, 80), (19, 4, 4)))
def test_pattern_playouts_slots_chunks_shards_and_ownership(case):
    _run(STACK_PLAYOUTS.replace('@CASE@', repr(case)))


@pytest.mark.parametrize('case', ((5, 6, 4), (9, 4, 2), (7, 3, 2)))      # (19x19: the guarded call below, against the same expectation)
def test_pattern_move_playouts_and_flat_mc(case):
    _run(STACK_MOVES.replace('@CASE@', repr(case)))


@pytest.mark.parametrize('case', ((5, 5, 10, 4), (9, 3, 6, 4), (19, 2, 3, 2)))
def test_pattern_uct_with_the_whole_tree(case):
    _run(STACK_UCT.replace('@CASE@', repr(case)))


def test_pattern_puct_over_the_playout_evaluator():
    _run(STACK_PUCT)


def test_policies_0_to_2_through_policy3_equal_policy2_and_pattern_changes_the_games():
    _run(FORWARD)


@pytest.mark.parametrize('N', SIZES)
def test_playouts_every_size_against_the_restatement(N):
    import mc_cases as cs
    import mc_expect as mc
    import mc_pattern_expect as mq
    from gymgo_amd import gogame
    roots = cs.playout_roots(N)[:4]
    K = 4 if N <= 13 else 2
    cap = cs.full_cap(N)
    want = mq.expected_playouts_pattern(roots, K, cap, komi=0.5)
    got = gogame.batch_playouts(mc.to_dev(roots), K, max_plies=cap, komi=0.5, slots=5, chunk_plies=32, policy='pattern')
    mc.check(got, want, mc.KEYS, N)


# ---------------------------------------------------------------- guards
def _arena_views(specs, k, device='cuda'):
    """An arena with one view per (name, shape, dtype, readonly) of specs, buffer j at the (k + j)-th residue its element size allows."""
    import guard_arena as ga
    arena = ga.Arena(sum(ga.footprint(shape, dtype) for _, shape, dtype, _ in specs) + 64, device)
    views = {}
    for j, (name, shape, dtype, ro) in enumerate(specs):
        res = ga.residues(dtype)
        views[name] = arena.take(name, shape, dtype, res[(k + j) % len(res)], readonly=ro)
    return arena, views


@pytest.mark.parametrize('N', (2, 9, 19))
def test_guards_the_five_calls_at_every_start_residue(N):
    """gg_batch_patterns, gg_batch_patterns_tracked, gg_batch_rollout_tracked_policy3, gg_playouts_advance_policy3 and
    gg_move_playouts_advance_policy3 with every buffer inside a guarded arena, every buffer at every start residue of its element
    size: nothing outside the buffers and no read-only buffer changes, and the results are those of the first round."""
    import mc_cases as cs
    import mc_expect as mc
    import mc_pattern_expect as mq
    from gymgo_amd import _lib, gogame
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    B, W, plies = 11, 5 * N + 1, 9
    states, last = mq.rollout_batch(N, B)
    st0 = mc.to_dev(states)
    tr0 = gogame.batch_track(st0)
    la0 = torch.from_numpy(last).cuda()
    want_planes = torch.from_numpy(_want_planes(states, last)).cuda()
    rng0 = gogame.rng_seed(B, 21, 0, 'cuda')
    wst, wrng, wlast, _ = mq.pattern_rollout(states, rng0.cpu().numpy().view(np.uint64), plies, False, last=last)
    roots = cs.playout_roots(N)[:3]
    R, K, S, chunk = len(roots), 2, 4, 8
    cap = min(cs.full_cap(N), 160)      # (19x19: playouts cut at 160 plies count as unfinished - the buffers are what is looked at)
    rt0 = gogame.batch_track(mc.to_dev(roots))
    want_po = mq.expected_playouts_pattern(roots, K, cap, komi=0.5, base_seed=77, with_ownership=True)
    want_mv = mq.expected_move_playouts_pattern(roots[:1], 1, cap, komi=0.5, base_seed=78)
    A = N * N + 1
    for k in range(16):      # 16 / 8 / 4 / 2 residues of 1- / 2- / 4- / 8-byte elements: every buffer meets every one of its own
        s = _stream()
        # the planes, both forms, with an orientation
        arena, v = _arena_views([('states', (B, 6, N, N), u8, True), ('tracked', (B, W), i32, True), ('last', (B,), i32, True),
                                 ('orient', (B,), i32, True), ('out', (B, 2, N, N), u8, False), ('out2', (B, 2, N, N), u8, False)], k)
        v['states'].copy_(st0); v['tracked'].copy_(tr0); v['last'].copy_(la0); v['orient'].zero_()
        arena.snapshot()
        _lib.call('gg_batch_patterns', v['states'], v['last'], v['orient'], v['out'], 3, B, N, s)
        _lib.call('gg_batch_patterns_tracked', v['tracked'], v['last'], v['orient'], v['out2'], 3, B, N, s)
        assert arena.violations() == [], (N, k, 'planes')
        assert torch.equal(v['out'], want_planes) and torch.equal(v['out2'], want_planes), (N, k)
        # the rollout: last_actions in and out
        arena, v = _arena_views([('tracked', (B, W), i32, False), ('rng', (B,), i64, False), ('last_actions', (B,), i32, False),
                                 ('steps_done', (B,), i64, False)], k)
        v['tracked'].copy_(tr0); v['rng'].copy_(rng0); v['last_actions'].copy_(la0); v['steps_done'].zero_()
        arena.snapshot()
        _lib.call('gg_batch_rollout_tracked_policy3', v['tracked'], v['rng'], v['last_actions'], v['steps_done'], B, N, plies, 0, 3, s)
        assert arena.violations() == [], (N, k, 'rollout')
        assert np.array_equal(gogame.batch_untrack(v['tracked'].clone()).cpu().numpy(), wst), (N, k)
        assert np.array_equal(v['rng'].cpu().numpy().view(np.uint64), wrng) and np.array_equal(v['last_actions'].cpu().numpy(), wlast), (N, k)
        # the playout queue
        arena, v = _arena_views([('roots', (R, W), i32, True), ('slots', (S, W), i32, False), ('rng', (S,), i64, False),
                                 ('plies', (S,), i64, False), ('job', (S,), i64, False), ('counter', (2,), i64, False),
                                 ('counts', (R, 4), i32, False), ('sums', (R, 2), i64, False),
                                 ('ownership', (R, 2, N, N), i32, False), ('last', (S,), i32, False)], k)
        v['roots'].copy_(rt0)
        head = (v['roots'], R, N, K, 0, 77, cap, chunk)
        bufs = (v['slots'], v['rng'], v['plies'], v['job'], S, v['counter'], v['counts'], v['sums'], v['ownership'])
        rounds = (-(-R * K // S) + 1) * (cap // chunk) + 2
        arena.snapshot()
        _lib.call('gg_playouts_begin', *head, *bufs, s)
        v['last'].fill_(-1)
        _lib.call('gg_playouts_advance_policy3', *head, 0.5, rounds, 3, *bufs, v['last'], s)
        assert arena.violations() == [], (N, k, 'playouts')
        c = v['counter'].cpu().numpy()
        assert c[0] == c[1] and bool((v['last'] == -1).all())                                  # every job done, every slot emptied
        assert np.array_equal(v['counts'][:, 0].cpu().numpy(), want_po['black_wins']), (N, k)
        assert np.array_equal(v['sums'][:, 1].cpu().numpy(), want_po['plies_sum']), (N, k)
        assert np.array_equal(v['ownership'].cpu().numpy(), want_po['ownership']), (N, k)
        # the first-move queue on one root
        T = int(want_mv['legal'].sum())
        plan = torch.from_numpy(np.flatnonzero(want_mv['legal'][0]).astype(np.int32)).cuda()
        arena, v = _arena_views([('roots', (1, W), i32, True), ('plan', (max(T, 1),), i32, True), ('slots', (S, W), i32, False),
                                 ('rng', (S,), i64, False), ('plies', (S,), i64, False), ('job', (S,), i64, False),
                                 ('counter', (2,), i64, False), ('counts', (1, A, 4), i32, False), ('sums', (1, A, 2), i64, False),
                                 ('last', (S,), i32, False)], k)
        v['roots'].copy_(rt0[:1])
        if T:
            v['plan'].copy_(plan)
        head = (v['roots'], 1, N, v['plan'], T, 1, 0, 78, cap, chunk)
        bufs = (v['slots'], v['rng'], v['plies'], v['job'], S, v['counter'], v['counts'], v['sums'])
        rounds = (-(-T // S) + 1) * (cap // chunk) + 2
        arena.snapshot()
        _lib.call('gg_move_playouts_begin', *head, *bufs, s)
        v['last'].fill_(-1)
        _lib.call('gg_move_playouts_advance_policy3', *head, 0.5, rounds, 3, *bufs, v['last'], s)
        assert arena.violations() == [], (N, k, 'move playouts')
        c = v['counter'].cpu().numpy()
        assert c[0] == c[1] and bool((v['last'] == -1).all())
        assert np.array_equal(v['counts'][0, :, 0].cpu().numpy(), want_mv['black_wins'][0]), (N, k)
        assert np.array_equal(v['sums'][0, :, 1].cpu().numpy(), want_mv['plies_sum'][0]), (N, k)
