"""-m gpu: the move log of the rollouts, the AMAF statistics of the playout queue and RAVE in the UCT search on the device
(include/gymgo_amd_amaf.h), bit-exact against tests/mc_amaf_expect.py, whose cases tests/test_amaf_host.py holds to
their premises on the CPU.

The both-families test sizes the library for FOUR compute units (GYMGO_AMD_CUS=4, read once per process: a process of its own, as
tests/test_gpu_tactics.py does), so that 19x19 batches above 512 games and 9x9 / 13x13 batches above 636 take the log variants of
k_rollout5 for launches of >= 8 plies, small batches take k_rollout_lat_log where the uniform path takes k_rollout_lat, and the
band in between - k_rollout4's for the uniform policy - takes k_rollout_lat_log too."""
import math
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

import mc_amaf_expect as ma   # noqa: E402
import mc_expect as mc        # noqa: E402

SIZES = tuple(range(2, 20))


def _stream():
    from gymgo_amd import _lib
    return _lib.stream_ptr(torch.device('cuda', torch.cuda.current_device()))


def _rng_dev(rng):
    return torch.from_numpy(np.asarray(rng, np.uint64).view(np.int64).copy()).cuda()


def check_log_launch(states, rng, acts, plies, policy, tag):
    """One launch of `plies` plies with the log against gg_batch_rollout_tracked_policy2 on copies (boards, generators, step counts,
    last actions) and against the restatement's sequence (the played entries; the others keep 0xFFFF)."""
    from gymgo_amd import _lib, gogame
    B, N = states.shape[0], states.shape[-1]
    st = torch.from_numpy(np.array(states, np.uint8)).cuda()      # (a copy: the cases are read-only)
    tr, tr2 = gogame.batch_track(st), gogame.batch_track(st)
    r1, r2 = _rng_dev(rng), _rng_dev(rng)
    la1, la2 = (torch.full((B,), -9, dtype=torch.int32, device='cuda') for _ in range(2))
    sd1, sd2 = (torch.full((B,), 3, dtype=torch.int64, device='cuda') for _ in range(2))
    log = torch.full((B, plies), ma.UNWRITTEN, dtype=torch.int16, device='cuda')
    gogame.batch_rollout_tracked_log(tr, r1, plies, log, la1, sd1, policy=ma.POLICIES[policy])
    _lib.call('gg_batch_rollout_tracked_policy2', tr2, r2, la2, sd2, B, N, plies, 0, policy, _stream())
    for name, x, y in (('boards', tr, tr2), ('rng', r1, r2), ('last_actions', la1, la2), ('steps_done', sd1, sd2)):
        assert torch.equal(x, y), (tag, name)
    want = acts[:, :plies].astype(np.int16)                   # -1 where nothing was played = the bytes the log held
    got = log.cpu().numpy()
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (tag, bad[:6].tolist(), got[bad[:1]], want[bad[:1]])
    assert np.array_equal(sd1.cpu().numpy() - 3, (want >= 0).sum(axis=1))


@pytest.mark.parametrize('policy', (0, 1, 2))
@pytest.mark.parametrize('N', SIZES)
def test_log_rollout_every_size_and_policy(N, policy):
    states, rng, acts = ma.log_case(N, policy)
    assert (acts[:, 0] >= 0).any() and (acts[:, 0] < 0).any()
    for plies in ma.LOG_PLIES:
        check_log_launch(states, rng, acts, plies, policy, (N, policy, plies))


FAMILIES = r'''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
from gymgo_amd import _lib
from oracle import c_oracle
import mc_amaf_expect as ma
import test_gpu_amaf as tg
assert _lib.lib().gg_device_cus() == 4
# 4 CUs.  19x19: up to 64 games k_rollout_lat_log (the uniform path: k_rollout_lat), 65 .. 512 the band of k_rollout4 (here:
# k_rollout_lat_log), from 513 games and 8 plies on the log variants of k_rollout5 - 513 games are 29 groups of 18 boards, the last
# one of 9: a ragged last wave.  9x9 / 13x13: the band up to 636 games, k_rollout5's variants above
for N, sizes in ((19, (33, 200, 513)), (9, (300, 637)), (13, (255, 701))):
    for B in sizes:
        for policy in (0, 1, 2):
            states = ma.log_boards(N, B)
            rng = c_oracle.rng_seed(7000 + B + policy, B)
            _, _, acts, _ = ma.play_sequences(states, rng, 33, policy)
            for plies in (7, 33):       # (7: below k_rollout5's eight plies, every batch on the one-row-per-lane kernel)
                tg.check_log_launch(states, rng, acts, plies, policy, (N, B, policy, plies))
torch.cuda.synchronize()
print('AMAF OK')
''' % (ROOT, os.path.join(ROOT, 'tests'))


def test_log_rollout_both_families_the_band_and_a_ragged_last_wave():
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    p = subprocess.run([sys.executable, '-c', FAMILIES], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'AMAF OK' in p.stdout


# ---------------------------------------------------------------- batch_playouts(amaf=True)
FIELDS = mc.KEYS + ('ownership', 'amaf')


def _playouts(N, policy, cut, dev, **kw):
    from gymgo_amd import gogame
    cap = ma.PO_CUT[N] if cut else ma.cs.full_cap(N)
    kw.setdefault('chunk_plies', 32 if not cut else min(32, cap))
    return gogame.batch_playouts(dev, ma.PO_K, max_plies=cap, komi=ma.PO_KOMI, seed=ma.PO_SEED + N, ownership=True,
                                 policy=ma.POLICIES[policy], **kw)


@pytest.mark.parametrize('N', SIZES)
def test_playouts_amaf_every_size(N):
    from gymgo_amd import gogame
    roots = ma.playout_roots(N)
    dev = mc.to_dev(roots)
    want = ma.playout_case(N)
    got = _playouts(N, 0, False, dev, amaf=True)
    assert got.amaf.dtype == torch.int32 and tuple(got.amaf.shape) == (3, 2, 3, N, N)
    mc.check(got, want, FIELDS, N)
    plain = _playouts(N, 0, False, dev)
    assert type(plain) is gogame.Playouts and type(got) is gogame.PlayoutsAmaf
    for k in mc.KEYS + ('ownership',):
        assert torch.equal(getattr(got, k), getattr(plain, k)), (N, k)
    assert bool((dev == mc.to_dev(roots)).all())
    if N == 4:      # NumPy in, NumPy out; the single-state form
        mc.check(_playouts(N, 0, False, roots, amaf=True), want, FIELDS, 'numpy')
        one = gogame.playouts(roots[1], ma.PO_K, max_plies=ma.cs.full_cap(N), komi=ma.PO_KOMI, seed=ma.PO_SEED + N, first_root=1, amaf=True)
        assert np.array_equal(one.amaf, want['amaf'][1])


@pytest.mark.parametrize('N', ma.PO_SIZES_MORE)
def test_playouts_amaf_slots_chunks_shards_cut_off_and_policies(N):
    roots = ma.playout_roots(N)
    dev = mc.to_dev(roots)
    want = ma.playout_case(N)
    for slots in (4, 15, None):
        for chunk in (8, 32):
            mc.check(_playouts(N, 0, False, dev, amaf=True, slots=slots, chunk_plies=chunk), want, FIELDS, (N, slots, chunk))
    a = _playouts(N, 0, False, dev[:1], amaf=True)
    b = _playouts(N, 0, False, dev[1:], amaf=True, first_root=1, slots=7)
    for k in FIELDS:
        assert np.array_equal(np.concatenate([mc.to_np(getattr(a, k)), mc.to_np(getattr(b, k))]), want[k]), (N, k)
    cut = ma.playout_case(N, 0, True)
    assert cut['unfinished'].sum() > 0
    for slots, chunk in ((None, ma.PO_CUT[N]), (4, 8)):
        mc.check(_playouts(N, 0, True, dev, amaf=True, slots=slots, chunk_plies=chunk), cut, FIELDS, (N, 'cut', slots, chunk))
    for policy in (1, 2):
        mc.check(_playouts(N, policy, False, dev, amaf=True, slots=6, chunk_plies=16), ma.playout_case(N, policy), FIELDS, (N, policy))


# ---------------------------------------------------------------- batch_uct(rave_equiv=...)
def _uct(N, c, dev, **kw):
    from gymgo_amd import gogame
    return gogame.batch_uct(dev, ma.RAVE_I, ma.RAVE_K, c=c, komi=ma.RAVE_KOMI, seed=900 + N, tree=True, **kw)


@pytest.mark.parametrize('c', ma.RAVE_CS)
@pytest.mark.parametrize('N', ma.RAVE_SIZES)
def test_uct_rave_whole_tree(N, c):
    from gymgo_amd import gogame
    roots = ma.rave_roots(N)
    dev = mc.to_dev(roots)
    want = ma.rave_case(N, c)
    got = _uct(N, c, dev, rave_equiv=ma.RAVE_EQUIV, fpu=ma.RAVE_FPU)
    assert type(got) is gogame.UctRave and type(got.tree) is gogame.UctRaveTree
    mc.check(got, want, ma.RAVE_ROOT_KEYS, (N, c))
    mc.check(got.tree, want['tree'], ma.RAVE_TREE_KEYS, (N, c))
    assert np.array_equal(mc.to_np(gogame.uct_actions(dev, ma.RAVE_I, ma.RAVE_K, c=c, komi=ma.RAVE_KOMI, seed=900 + N, rave_equiv=ma.RAVE_EQUIV,
                                                      fpu=ma.RAVE_FPU, slots=5, chunk_plies=16)), mc.most_visited(want))
    assert bool((dev == mc.to_dev(roots)).all())
    if c == 0.0:      # rave_equiv=None is today's search: its record type, its trees
        plain = _uct(N, math.sqrt(2), dev, rave_equiv=None)
        assert type(plain) is gogame.Uct and type(plain.tree) is gogame.UctTree
        p = ma.plain_case(N, math.sqrt(2))
        mc.check(plain, p, mc.ROOT_KEYS, (N, 'plain'))
        mc.check(plain.tree, p['tree'], mc.TREE_KEYS, (N, 'plain'))


def test_uct_rave_past_capacity():
    """PAST_I + PAST_EXTRA iterations through the entry points on trees with room for PAST_I + 1 nodes: once a tree is full, a
    winner without a child leaves the node it was found at to be evaluated as it is."""
    from gymgo_amd import _lib, gogame
    N, I, K = ma.PAST_N, ma.PAST_I, ma.RAVE_K
    want = ma.past_capacity_case()
    roots = ma.rave_roots(N)
    R, W, A, NN = len(roots), 5 * N + 1, N * N + 1, I + 1
    tr = gogame.batch_track(mc.to_dev(roots))
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device='cuda')
    boards, child, links, stats, nodes = i32(R, NN, W), i32(R, NN, A), i32(R, NN, 2), i32(R, NN, 4), i32(R)
    leaf, move, leaf_id = i32(R, W), i32(R), i32(R)
    totals = torch.zeros((R, 2), dtype=torch.int64, device='cuda')
    node_amaf = torch.zeros((R, NN, N * N, 2), dtype=torch.int32, device='cuda')
    L = torch.from_numpy(mc.log_table(I, K)).cuda()
    S, chunk, cap = 6, 32, ma.cs.full_cap(N)
    pbufs, abufs = gogame._playout_buffers(R, S, N, 'cuda'), gogame._amaf_buffers(R, S, N, chunk, 'cuda')
    s = _stream()
    _lib.call('gg_uct_begin', tr, R, N, I, K, boards, child, links, stats, nodes, s)
    for i in range(I + ma.PAST_EXTRA):
        _lib.call('gg_uct_select_rave', R, N, I, K, 0.5, ma.RAVE_EQUIV, ma.RAVE_FPU, L, boards, child, links, stats, node_amaf, nodes, leaf,
                  move, leaf_id, s)
        _lib.call('gg_batch_play_moves_tracked', leaf, move, None, R, N, 1, s)
        gogame._run_playouts(leaf, R, N, K, cap, ma.RAVE_KOMI, gogame._uct_seed(31, i), 0, False, S, chunk, torch.device('cuda', 0), pbufs, 0,
                             amaf=abufs)
        _lib.call('gg_uct_backup_rave', R, N, I, K, pbufs[5], pbufs[6], abufs[3], totals, boards, links, stats, node_amaf, leaf, move,
                  leaf_id, s)
    t = want['tree']
    assert np.array_equal(nodes.cpu().numpy(), want['nodes'])
    assert np.array_equal(links.cpu().numpy(), np.stack([t['parent'], t['action']], axis=-1))
    assert np.array_equal(stats.cpu().numpy(), np.stack([t[k] for k in ('visits', 'black_wins', 'white_wins', 'draws')], axis=-1))
    assert np.array_equal(node_amaf.cpu().numpy(), t['node_amaf'])
    assert np.array_equal(totals.cpu().numpy(), np.stack([want['unfinished'], want['plies_sum']], axis=-1))


def test_python_api_checks_its_rave_and_amaf_arguments():
    from gymgo_amd import gogame
    st = np.zeros((2, 6, 5, 5), np.uint8)
    for kw in ({'rave_equiv': 0}, {'rave_equiv': -2.0}, {'rave_equiv': float('nan')}, {'rave_equiv': 10, 'fpu': float('inf')},
               {'rave_equiv': 10, 'chunk_plies': 8192, 'max_plies': 8192}):
        with pytest.raises(ValueError):
            gogame.batch_uct(st, 4, 2, **kw)
    with pytest.raises(ValueError):
        gogame.batch_uct(st, 1 << 20, 1 << 10, rave_equiv=10)
    with pytest.raises(ValueError):
        gogame.batch_playouts(st, 2, amaf=True, chunk_plies=8192, max_plies=8192)
    with pytest.raises(ValueError):
        gogame.batch_rollout_tracked_log(gogame.batch_track(mc.to_dev(st)), gogame.rng_seed(2, 1, 0, 'cuda'), 4,
                                         torch.zeros((2, 5), dtype=torch.int16, device='cuda'))


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


def _residue_rounds():
    return range(16)      # 16 / 8 / 4 / 2 residues of 1- / 2- / 4- / 8-byte elements: every buffer meets every one of its own


@pytest.mark.parametrize('N', (2, 9, 19))
def test_guards_log_rollout(N):
    from gymgo_amd import _lib, gogame
    B, plies, W = 11, 9, 5 * N + 1
    states, rng, acts = ma.log_case(N, 2)
    states, rng, acts = states[:B], rng[:B], acts[:B]
    tr0 = gogame.batch_track(mc.to_dev(states))
    for policy in (0, 2):
        seq = acts if policy == 2 else ma.play_sequences(states, rng, plies, 0)[2]
        plain = None
        for k in _residue_rounds():
            arena, v = _arena_views([('tracked', (B, W), torch.int32, False), ('rng', (B,), torch.int64, False),
                                     ('last_actions', (B,), torch.int32, False), ('steps_done', (B,), torch.int64, False),
                                     ('log', (B, plies), torch.int16, False)], k)
            v['tracked'].copy_(tr0)
            v['rng'].copy_(_rng_dev(rng))
            v['steps_done'].zero_()
            v['log'].fill_(ma.UNWRITTEN)
            arena.snapshot()
            _lib.call('gg_batch_rollout_tracked_log', v['tracked'], v['rng'], v['last_actions'], v['steps_done'], B, N, plies, policy,
                      v['log'], _stream())
            assert arena.violations() == [], (N, policy, k)
            out = tuple(v[n].clone() for n in ('tracked', 'rng', 'last_actions', 'steps_done', 'log'))
            assert np.array_equal(out[4].cpu().numpy(), seq[:, :plies].astype(np.int16)), (N, policy, k)
            plain = plain or out
            for x, y in zip(out, plain):
                assert torch.equal(x, y), (N, policy, k)


@pytest.mark.parametrize('N', (2, 9, 19))
def test_guards_playouts_advance_amaf(N):
    from gymgo_amd import _lib, gogame
    roots = ma.playout_roots(N)
    R, K, S, chunk, W = 3, ma.PO_K, 4, 8, 5 * N + 1
    cap = ma.cs.full_cap(N)
    want = ma.playout_case(N)
    tr0 = gogame.batch_track(mc.to_dev(roots))
    rounds = (-(-R * K // S) + 1) * (cap // chunk) + 2
    for k in _residue_rounds():
        arena, v = _arena_views([('roots', (R, W), torch.int32, True), ('slots', (S, W), torch.int32, False), ('rng', (S,), torch.int64, False),
                                 ('plies', (S,), torch.int64, False), ('job', (S,), torch.int64, False), ('counter', (2,), torch.int64, False),
                                 ('counts', (R, 4), torch.int32, False), ('sums', (R, 2), torch.int64, False),
                                 ('ownership', (R, 2, N, N), torch.int32, False), ('log', (S, chunk), torch.int16, False),
                                 ('first', (S, 2, N), torch.int32, False), ('mark', (S,), torch.int64, False),
                                 ('amaf', (R, 2, 3, N, N), torch.int32, False)], k)
        v['roots'].copy_(tr0)
        head = (v['roots'], R, N, K, 0, ma.PO_SEED + N, cap, chunk)
        bufs = (v['slots'], v['rng'], v['plies'], v['job'], S, v['counter'], v['counts'], v['sums'], v['ownership'])
        arena.snapshot()
        s = _stream()
        _lib.call('gg_playouts_begin', *head, *bufs, s)
        for n in ('first', 'mark', 'amaf'):
            v[n].zero_()
        _lib.call('gg_playouts_advance_amaf', *head, ma.PO_KOMI, rounds, 0, *bufs, v['log'], v['first'], v['mark'], v['amaf'], s)
        assert arena.violations() == [], (N, k)
        c = v['counter'].cpu().numpy()
        assert c[0] == c[1]                                   # every job done
        assert np.array_equal(v['amaf'].cpu().numpy(), want['amaf']), (N, k)
        assert np.array_equal(v['ownership'].cpu().numpy(), want['ownership']) and np.array_equal(v['counts'][:, 0].cpu().numpy(), want['black_wins'])
        assert not v['first'].any() and not v['mark'].any()   # every slot emptied


@pytest.mark.parametrize('N', (2, 9, 19))
def test_guards_uct_rave_select_and_backup(N):
    """Three iterations of the RAVE search with every buffer of select and backup inside the arena; the tree equals the one the
    Python API builds with its own buffers."""
    from gymgo_amd import _lib, gogame
    roots = ma.rave_roots(N)
    R, I, K, W, A, NN, P = len(roots), 3, ma.RAVE_K, 5 * N + 1, N * N + 1, 4, N * N
    dev = mc.to_dev(roots)
    ref = gogame.batch_uct(dev, I, K, c=0.5, komi=ma.RAVE_KOMI, seed=5, tree=True, rave_equiv=ma.RAVE_EQUIV, fpu=0.5)
    tr0 = gogame.batch_track(dev)
    S, chunk, cap = 5, 32, ma.cs.full_cap(N)
    i32, i64 = torch.int32, torch.int64
    for k in _residue_rounds():
        arena, v = _arena_views([('log_table', (NN,), torch.float64, True), ('boards', (R, NN, W), i32, False), ('child', (R, NN, A), i32, False),
                                 ('links', (R, NN, 2), i32, False), ('stats', (R, NN, 4), i32, False), ('node_amaf', (R, NN, P, 2), i32, False),
                                 ('nodes', (R,), i32, False), ('leaf', (R, W), i32, False), ('move', (R,), i32, False),
                                 ('leaf_id', (R,), i32, False), ('counts', (R, 4), i32, False), ('sums', (R, 2), i64, False),
                                 ('amaf', (R, 2, 3, N, N), i32, False), ('totals', (R, 2), i64, False)], k)
        v['log_table'].copy_(torch.from_numpy(mc.log_table(I, K)))
        v['node_amaf'].zero_()
        v['totals'].zero_()
        s = _stream()
        _lib.call('gg_uct_begin', tr0, R, N, I, K, v['boards'], v['child'], v['links'], v['stats'], v['nodes'], s)
        pbufs = gogame._playout_buffers(R, S, N, 'cuda')[:5] + (v['counts'], v['sums'])
        abufs = gogame._amaf_buffers(R, S, N, chunk, 'cuda')[:3] + (v['amaf'],)
        for i in range(I):
            # select: the tree's boards and the AMAF pairs are inputs (a new node's stats are zeroed there)
            for n in ('boards', 'node_amaf', 'counts', 'sums', 'amaf', 'totals'):
                arena.set_readonly(n, True)
            arena.snapshot()
            _lib.call('gg_uct_select_rave', R, N, I, K, 0.5, ma.RAVE_EQUIV, 0.5, v['log_table'], v['boards'], v['child'], v['links'], v['stats'],
                      v['node_amaf'], v['nodes'], v['leaf'], v['move'], v['leaf_id'], s)
            assert arena.violations() == [], (N, k, i, 'select')
            for n in ('boards', 'node_amaf', 'counts', 'sums', 'amaf', 'totals'):
                arena.set_readonly(n, False)
            _lib.call('gg_batch_play_moves_tracked', v['leaf'], v['move'], None, R, N, 1, s)
            gogame._run_playouts(v['leaf'], R, N, K, cap, ma.RAVE_KOMI, gogame._uct_seed(5, i), 0, False, S, chunk, torch.device('cuda', 0),
                                 pbufs, 0, amaf=abufs)
            # backup: the counts, the links, the leaf and the child table are inputs
            for n in ('counts', 'sums', 'amaf', 'links', 'leaf', 'move', 'leaf_id', 'child', 'nodes'):
                arena.set_readonly(n, True)
            arena.snapshot()
            _lib.call('gg_uct_backup_rave', R, N, I, K, v['counts'], v['sums'], v['amaf'], v['totals'], v['boards'], v['links'], v['stats'],
                      v['node_amaf'], v['leaf'], v['move'], v['leaf_id'], s)
            assert arena.violations() == [], (N, k, i, 'backup')
            for n in ('counts', 'sums', 'amaf', 'links', 'leaf', 'move', 'leaf_id', 'child', 'nodes'):
                arena.set_readonly(n, False)
        assert torch.equal(v['node_amaf'], ref.tree.node_amaf), (N, k)
        assert torch.equal(v['links'][..., 0], ref.tree.parent) and torch.equal(v['links'][..., 1], ref.tree.action), (N, k)
        assert torch.equal(v['stats'][..., 0], ref.tree.visits) and torch.equal(v['nodes'], ref.nodes), (N, k)
