"""-m gpu: the Monte Carlo and tree-search stack at EVERY board size from 2 to 19, bit for bit against its restatements - the playout
queue (gg_po.h), flat Monte Carlo, UCT (gg_uct.h), the no_eye_fill rollout, k_eye_mask, and PUCT with leaves, tree reuse, root
noise and root policy (gg_puct.h).  The tests of those pieces run at 5, 7, 9, 13 and 19; what the other sizes add:

- the instantiations of row capacity 13 and 19 on boards that do not fill their rows (10 .. 12, 14 .. 18: the runtime N, full =
  (1 << N) - 1, r < N) - k_po_harvest for both queues, lat_areas inside k_puct_backup at ended leaves, lat_play_full in the refill
  of flat Monte Carlo, the policy form of k_rollout_lat;
- k_puct_advance's row moves (dwordx4 and a tail of words % 4) on rows of A = N^2 + 1 and W = 5 N + 1 words: every even N has
  A % 4 == 1 and W % 4 in {1, 3}, so row starts fall on all four word alignments (odd N: A % 4 == 2, W % 4 in {0, 2});
- the lane-stride loops over the actions at A = 5 (N = 2), A = 65 (N = 8: one full round of 64 lanes, then the pass alone) and
  A = 257 (N = 16);
- the harvest behind k_rollout4, which serves the queue's chunks at every size but 9, 13 and 19 once the slots outnumber
  k_rollout_lat's share;
- UCT's argmax descent, which starts only where every legal action of a node has a child: the late roots of tests/mc_cases.py
  have at most six legal points.

The roots are those of tests/mc_cases.py; tests/test_mc_cases_host.py asserts on the CPU that they are what these cases need.
The queue stack runs in a child process per size with the library sized for ONE compute unit (GYMGO_AMD_CUS=1, read once per
process): 24 slots then take k_rollout_lat up to 13x13 and k_rollout4 above (tracked boards: 64 / 16 games per CU), 200 slots
k_rollout5 at 9 / 13 / 19 and k_rollout4 elsewhere (gg_kernels.hip: use_lat, use_rollout5); a slot count is capped at the number
of jobs, so the searches' few leaves always take k_rollout_lat.  PUCT runs in the test's own process.  Integers are compared
with np.array_equal, floats as bit patterns: no tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mc_cases as cs
import mc_expect as mc
import mc_puct_expect as pe
import mc_puct_leaves_expect as pl
import mc_puct_selfplay_expect as ps
import test_gpu_puct_advance as tpa
import test_gpu_puct_selfplay as tps

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = list(cs.SIZES)

QUEUE = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
import numpy as np
import torch
from gymgo_amd import gogame, _lib
from oracle import c_oracle
import mc_cases as cs
import mc_expect as mc
import mc_policy_expect as mp
N = int(sys.argv[1])
assert _lib.lib().gg_device_cus() == 1
K, CAP = cs.PLAYOUT_K, cs.full_cap(N)
OWN = mc.KEYS + ('ownership',)

# ---- batch_playouts: both policies, the full cap and a cap of one chunk, both slot counts, both chunk lengths; shards
roots = cs.playout_roots(N)
dev = mc.to_dev(roots)
R = roots.shape[0]
for policy, expected in (('uniform', mc.expected_playouts), ('no_eye_fill', mp.expected_playouts_policy)):
    want = {cap: expected(roots, K, cap, komi=0.5, with_ownership=True) for cap in (CAP,) + cs.CHUNKS}
    for slots in cs.SLOTS:
        for chunk in cs.CHUNKS:
            for cap in (CAP, chunk):
                got = gogame.batch_playouts(dev, K, max_plies=cap, komi=0.5, ownership=True, slots=slots, chunk_plies=chunk, policy=policy)
                mc.check(got, want[cap], OWN, ('playouts', policy, slots, chunk, cap))
    cut = R // 3
    a = gogame.batch_playouts(dev[:cut], K, max_plies=CAP, komi=0.5, ownership=True, slots=200, policy=policy)
    b = gogame.batch_playouts(dev[cut:], K, max_plies=CAP, komi=0.5, ownership=True, slots=24, first_root=cut, policy=policy)
    mc.check(gogame.Playouts(*[torch.cat([x, y]) for x, y in zip(a, b)]), want[CAP], OWN, ('playouts', policy, 'shards'))
assert bool((dev == mc.to_dev(roots)).all())

# ---- flat Monte Carlo: a mid-game root, a late root, a finished game; the legal mask and the plan order are in the comparison
roots = cs.stack(N, cs.move_names(N))
dev = mc.to_dev(roots)
want = mc.expected_move_playouts(roots, 2, CAP, komi=0.5, first_root=2)
assert want['legal'][:2].any(axis=1).all() and not want['legal'][2].any()
for slots in cs.SLOTS:
    for chunk in cs.CHUNKS:
        got = gogame.batch_move_playouts(dev, 2, max_plies=CAP, komi=0.5, first_root=2, slots=slots, chunk_plies=chunk)
        mc.check(got, want, ('legal',) + mc.KEYS, ('move playouts', slots, chunk))
act = gogame.flat_mc_actions(dev, 2, max_plies=CAP, komi=0.5, first_root=2, slots=200, chunk_plies=8)
choice = mc.flat_mc_choice(roots, want)
assert np.array_equal(mc.to_np(act), choice) and choice[2] == -1 and (choice[:2] >= 0).all(), (mc.to_np(act), choice)

# ---- UCT: the late roots (every action of a node gets a child: the argmax descent) and a mid-game root, the whole tree
roots = cs.stack(N, cs.search_names(N))
dev = mc.to_dev(roots)
want = mc.expected_uct(roots, cs.UCT_I, cs.UCT_K, max_plies=CAP, komi=0.5)
for slots in cs.SLOTS:
    for chunk in cs.CHUNKS:
        got = gogame.batch_uct(dev, cs.UCT_I, cs.UCT_K, max_plies=CAP, komi=0.5, slots=slots, chunk_plies=chunk, tree=True)
        mc.check(got, want, mc.ROOT_KEYS, ('uct', slots, chunk))
        mc.check(got.tree, want['tree'], mc.TREE_KEYS, ('uct tree', slots, chunk))
act = gogame.uct_actions(dev, cs.UCT_I, cs.UCT_K, max_plies=CAP, komi=0.5)
assert np.array_equal(mc.to_np(act), mc.most_visited(want))

# ---- the no_eye_fill rollout on tracked boards: boards, generators, last actions, steps_done after every launch
for B in (24, 200):
    states = cs.tiled(N, B)
    for auto_reset in (False, True):
        tr = gogame.batch_track(torch.from_numpy(states).cuda())
        rng = gogame.rng_seed(B, 300 + B + N, 0, 'cuda')
        want, want_rng = states.copy(), rng.cpu().numpy().view(np.uint64).copy()
        sd = torch.zeros(B, dtype=torch.int64, device='cuda')
        want_sd = np.zeros(B, np.int64)
        for F in (1, 7, 8, 32):
            la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
            gogame.batch_rollout_tracked(tr, rng, F, auto_reset, la, sd, policy='no_eye_fill')
            want, want_rng, want_last, steps = mp.policy_rollout(want, want_rng, F, auto_reset)
            want_sd += steps
            what = ('policy rollout', B, F, auto_reset)
            bad = np.flatnonzero((gogame.batch_untrack(tr).cpu().numpy() != want).reshape(B, -1).any(axis=1))
            assert len(bad) == 0, what + (bad[:6].tolist(),)
            assert np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng), what
            assert np.array_equal(la.cpu().numpy(), want_last), what
            assert np.array_equal(sd.cpu().numpy(), want_sd), what

# ---- the uniform rollout on 200 tracked boards, 9 plies (k_rollout5 at 9 / 13 / 19, k_rollout4 elsewhere): what the harvest reads -
# steps_done and the flag word (bit 0 turn, bit 1 the last move was a pass, bit 2 game over) - and the rest, against the oracle
B = 200
states = cs.tiled(N, B)
for auto_reset in (False, True):
    tr = gogame.batch_track(torch.from_numpy(states).cuda())
    rng = gogame.rng_seed(B, 500 + N, 0, 'cuda')
    rng0 = rng.cpu().numpy().view(np.uint64).copy()
    sd = torch.zeros(B, dtype=torch.int64, device='cuda')
    la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
    gogame.batch_rollout_tracked(tr, rng, 9, auto_reset, la, sd)
    want, want_rng, want_last = c_oracle.batch_rollout(states, rng0.copy(), 9, auto_reset)
    plies = mc.plies_from_rng(rng0, want_rng)
    assert (plies == 9).all() if auto_reset else ((plies == 0).any() and (plies == 9).any() and ((plies > 0) & (plies < 9)).any()), plies
    what = ('uniform rollout', auto_reset)
    assert np.array_equal(sd.cpu().numpy(), plies), what
    flags = want[:, 2, 0, 0].astype(np.int32) | (want[:, 4, 0, 0].astype(np.int32) << 1) | (want[:, 5, 0, 0].astype(np.int32) << 2)
    assert np.array_equal(tr[:, 5 * N].cpu().numpy(), flags), what
    assert np.array_equal(gogame.batch_untrack(tr).cpu().numpy(), want), what
    assert np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng) and np.array_equal(la.cpu().numpy(), want_last), what

# ---- the eye mask
roots = cs.stack(N)
eyes = gogame.batch_eye_mask(mc.to_dev(roots)).cpu().numpy()
assert eyes.shape == (len(roots), N, N) and np.array_equal(eyes.astype(bool), mp.eyes(roots)) and eyes.any()
torch.cuda.synchronize()
print('MC SIZES OK')
''' % {'root': os.path.dirname(HERE), 'here': HERE}


@pytest.mark.parametrize('size', SIZES)
def test_queue_stack_on_one_compute_unit(size):
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '1'
    p = subprocess.run([sys.executable, '-c', QUEUE, str(size)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'MC SIZES OK' in p.stdout


@pytest.mark.parametrize('size', SIZES)
def test_puct_whole_tree(size):
    """min(2 A, 80) iterations on every root, the hash and the hostile evaluator; the finished and the full boards again with
    komi 0 and -0.5: their values come from the device's own scoring (lat_areas at the runtime N)."""
    from gymgo_amd import gogame
    roots, I = cs.stack(size), cs.puct_iterations(size)
    dev = mc.to_dev(roots)
    for name in ('hash', 'hostile'):
        ev_np, ev_t = tpa.EVALUATORS[name]
        pe.check(gogame.batch_puct(dev, I, ev_t, komi=0.5, tree=True), pe.expected_puct(roots, I, ev_np, komi=0.5), tag=name)
    scored = cs.stack(size, cs.scored_names(size))
    for komi in (0.0, -0.5):
        pe.check(gogame.batch_puct(mc.to_dev(scored), I, pe.hash_evaluator_t, komi=komi, tree=True),
                 pe.expected_puct(scored, I, pe.hash_evaluator_np, komi=komi), tag=komi)
    assert bool((dev == mc.to_dev(roots)).all())


@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('L,T', [(4, 6), (64, 2)])
def test_puct_leaves(size, L, T):
    """Four leaves a round, and 64: more slots than a small board has legal actions - collisions and empty slots."""
    from gymgo_amd import gogame
    roots = cs.stack(size)
    want = pl.expected_puct_leaves(roots, T, L, pe.hash_evaluator_np, komi=0.5)
    pe.check(gogame.batch_puct(mc.to_dev(roots), T, pe.hash_evaluator_t, komi=0.5, tree=True, leaves=L), want, tag=(L, T))


@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('L,name', cs.TREE_CASES)
def test_puct_advance_whole_tree_buffers(size, L, name):
    """test_gpu_puct_advance.py's whole-buffer comparison around two advances, on this size's roots."""
    tpa.whole_tree_buffers(cs.stack(size), L, name, cs.ADVANCE_T, kinds=cs.advance_kinds(size, L))


@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('L,name', cs.TREE_CASES)
def test_puct_root_noise_and_root_policy(size, L, name):
    """test_gpu_puct_selfplay.py's noise and policy protocol on searched trees, on this size's roots."""
    tps.noise_and_policy_on_searched_trees(cs.stack(size), L, name, kinds=cs.noise_kinds(size, L))


@pytest.mark.parametrize('size', SIZES)
def test_puct_selfplay_record(size):
    """Three moves of self-play, four rounds each, the first two moves drawn from the visit counts."""
    from gymgo_amd import gogame
    roots = cs.stack(size)
    M, T = 3, 4
    noise = lambda mv, legal: tps._odd_noise(roots.shape[0], mc.to_np(legal).shape[1], salt=mv)
    kw = dict(komi=0.5, noise=noise, eps=0.25, sample_moves=2, seed=7, first_game=2)
    e = ps.expected_selfplay(roots, M, T, pe.hash_evaluator_np, **kw)
    assert (e['lengths'] == 0).any() and (e['lengths'] == M).any()
    got = gogame.puct_selfplay(mc.to_dev(roots), M, T, pe.hash_evaluator_t, record_states=True, **kw)
    tps._check_selfplay(got, e, size)
