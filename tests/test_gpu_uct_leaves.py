"""-m gpu: the UCT search with several leaves per root and round on the device (include/gymgo_amd_uct_leaves.h), bit for
bit against tests/mc_uct_leaves_expect.py - batch_uct(leaves=L, tree=True) in all three modes (plain, RAVE, RAVE with priors) at
every board size, ended nodes inside the tree, 64 slots, c in {0, sqrt 2, 1e6}, komi and first_root, shards, the playout queue's
slots and chunks, leaves=1 against leaves=None down to the tree buffers, NumPy and the forwarding calls, the entry points on the
test's own buffers (virt between select and backup, empty rows, a search past its capacity, sentinel tails; the one-leaf entry
points against the _leaves ones with L = 1 launch for launch), the five entry
points between guards at every start residue, and one child process with the library sized for one compute unit (later trips of
the grid-stride loops; the playout policies on both kernel families).  tests/test_uct_leaves_host.py holds the cases to their
premises on the CPU."""
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

import mc_cases as cs                # noqa: E402
import mc_expect as mc               # noqa: E402
import mc_uct_leaves_expect as ml    # noqa: E402


def _stream():
    from gymgo_amd import _lib
    return _lib.stream_ptr(torch.device('cuda', torch.cuda.current_device()))


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _mode_kw(mode, R, N):
    """batch_uct's keywords of a mode, from mc_uct_leaves_expect.mode_args."""
    from gymgo_amd import gogame
    rave, prior = ml.mode_args(mode, R, N)
    kw = {}
    if rave is not None:
        kw.update(rave_equiv=rave[0], fpu=rave[1])
    if prior is not None:
        kw.update(prior=gogame.UctPrior(*prior[0]), last_actions=prior[1])
    return kw


def _check(got, want, mode, tag):
    from gymgo_amd import gogame
    root_keys, tree_keys = ml.keys(mode)
    assert type(got) is (gogame.Uct if mode == 'plain' else gogame.UctRave), tag
    mc.check(got, want, root_keys, tag)
    mc.check(got.tree, want['tree'], tree_keys, (tag, 'tree'))


# ---------------------------------------------------------------- batch_uct(leaves=L) against the restatement
@pytest.mark.parametrize('N,mode,L', ml.all_size_cases())
def test_whole_tree_every_size(N, mode, L):
    from gymgo_amd import gogame
    T, K, cap, _ = ml.size_shape(N)
    roots, want = ml.size_case(N, mode, L)
    dev = mc.to_dev(roots)
    got = gogame.batch_uct(dev, T, K, c=ml.size_c(mode), max_plies=cap, komi=ml.KOMI, seed=ml.size_seed(N), leaves=L, tree=True,
                           **_mode_kw(mode, len(roots), N))
    _check(got, want, mode, (N, mode, L))
    assert tuple(got.tree.parent.shape) == (len(roots), T * L + 1)
    assert np.array_equal(mc.to_np(got.root_visits), K * want['live'].sum(axis=0))      # K times the non-empty slots
    assert bool((dev == mc.to_dev(roots)).all())


@pytest.mark.parametrize('L', (2, 4, 8))
@pytest.mark.parametrize('mode', ml.MODES)
def test_ended_nodes_inside_the_tree(mode, L):
    from gymgo_amd import gogame
    roots, want = ml.ended_case(mode, L)
    got = gogame.batch_uct(mc.to_dev(roots), ml.ENDED_T, ml.ENDED_K, c=0.3, max_plies=64, komi=ml.KOMI, seed=77, leaves=L, tree=True,
                           **_mode_kw(mode, len(roots), ml.ENDED_N))
    _check(got, want, mode, ('ended', mode, L))


@pytest.mark.parametrize('mode', ml.MODES)
def test_sixty_four_slots(mode):
    from gymgo_amd import gogame
    roots, want = ml.wide_case(mode)
    got = gogame.batch_uct(mc.to_dev(roots), 2, 2, c=ml.size_c(mode), max_plies=32, komi=ml.KOMI, seed=64, leaves=64, tree=True,
                           **_mode_kw(mode, len(roots), 9))
    _check(got, want, mode, ('wide', mode))


@pytest.mark.parametrize('c', (0.0, math.sqrt(2), ml.BIG_C))
@pytest.mark.parametrize('mode', ml.MODES)
def test_exploration_constants(mode, c):
    from gymgo_amd import gogame
    roots, want = ml.c_case(mode, c)
    got = gogame.batch_uct(mc.to_dev(roots), 6, 2, c=c, max_plies=64, komi=ml.KOMI, seed=91, leaves=8, tree=True,
                           **_mode_kw(mode, len(roots), 5))
    _check(got, want, mode, ('c', mode, c))


@pytest.mark.parametrize('mode', ml.MODES)
def test_komi_first_root_shards_slots_and_chunks(mode):
    """19x19 and 5x5: komi 7.5 and first_root = 3 against the restatement, whatever the slots and chunk_plies of the playout queue;
    shards by root concatenate to the whole."""
    from gymgo_amd import gogame
    for N, T, L, K, cap in ((19, 3, 4, 2, 64), (5, 5, 4, 3, 64)):
        roots = cs.stack(N, ('late0', 'mid0', 'late1', 'ended'))
        R, f0 = len(roots), 3
        rave, prior = ml.mode_args(mode, R, N)
        want = ml.expected_uct_leaves(roots, T, L, K, c=ml.size_c(mode), rave=rave, prior=prior, max_plies=cap, komi=7.5, base_seed=17,
                                      first_root=f0)
        dev = mc.to_dev(roots)
        kw = dict(c=ml.size_c(mode), max_plies=cap, komi=7.5, seed=17, leaves=L, tree=True)
        mk = _mode_kw(mode, R, N)
        for slots, chunk in ((None, 32), (3, 8), (11, 16)):
            got = gogame.batch_uct(dev, T, K, first_root=f0, slots=slots, chunk_plies=chunk, **kw, **mk)
            _check(got, want, mode, (N, mode, slots, chunk))
        parts = []
        for lo, hi in ((0, 1), (1, R)):
            pk = dict(mk)
            if 'last_actions' in pk:
                pk['last_actions'] = pk['last_actions'][lo:hi]
            parts.append(gogame.batch_uct(dev[lo:hi], T, K, first_root=f0 + lo, slots=5, **kw, **pk))
        root_keys, tree_keys = ml.keys(mode)
        for k in root_keys:
            assert np.array_equal(np.concatenate([mc.to_np(getattr(p, k)) for p in parts]), want[k]), (N, mode, k)
        for k in tree_keys:
            assert np.array_equal(np.concatenate([mc.to_np(getattr(p.tree, k)) for p in parts]), want['tree'][k]), (N, mode, k)


@pytest.mark.parametrize('N', (2, 9, 19))
def test_one_leaf_per_round_is_the_search_without_the_keyword(N):
    """leaves=1 against leaves=None, down to the tree buffers of the host loop.  Both run ONE kernel body (gg_uct.h, gg_prior.h):
    leaves=None its VL = false instantiations, leaves=1 the VL = true ones with L = 1 and every v = 0 where a score reads it.  What
    this guards is the `if (VL)` switches of that body - a difference of the several-leaves mode that is not under its switch, or a
    statement of the one-leaf mode that fell under one, shows here - not the agreement of two copies of the text."""
    from gymgo_amd import gogame
    roots = cs.stack(N, ('late0', 'mid0', 'empty', 'ended'))
    R, T, K, cap = len(roots), 12, 2, 64
    dev = mc.to_dev(roots)
    tr = gogame.batch_track(dev)
    for mode in ml.MODES:
        rave, prior = ml.mode_args(mode, R, N)
        pr = None if prior is None else (_i32([x for p in prior[0] for x in p]), _i32(prior[1]))
        args = (tr, R, N, T, K, ml.size_c(mode), cap, ml.KOMI, 5, 2, 16, 32, dev.device)
        a = gogame._run_uct(*args, rave=rave, prior=pr)
        b = gogame._run_uct(*args, rave=rave, prior=pr, leaves=1)
        assert len(a) == len(b) == (5 if rave is None else 6)
        for x, y in zip(a, b):
            assert x.shape == y.shape and torch.equal(x, y), (N, mode)
        mk = _mode_kw(mode, R, N)
        kw = dict(c=ml.size_c(mode), max_plies=cap, komi=ml.KOMI, seed=5, tree=True)
        p, q = gogame.batch_uct(dev, T, K, **kw, **mk), gogame.batch_uct(dev, T, K, leaves=1, **kw, **mk)
        root_keys, tree_keys = ml.keys(mode)
        for k in root_keys:
            assert torch.equal(getattr(p, k), getattr(q, k)), (N, mode, k)
        for k in tree_keys:
            assert torch.equal(getattr(p.tree, k), getattr(q.tree, k)), (N, mode, k)


def test_numpy_and_the_forwarding_calls():
    from gymgo_amd import gogame
    N, L = 5, 4
    T, K, cap, _ = ml.size_shape(N)
    for mode in ml.MODES:
        roots, want = ml.size_case(N, mode, L)
        mk = _mode_kw(mode, len(roots), N)
        kw = dict(c=ml.size_c(mode), max_plies=cap, komi=ml.KOMI, seed=ml.size_seed(N), leaves=L)
        got = gogame.batch_uct(np.array(roots), T, K, tree=True, **kw, **mk)
        assert isinstance(got.visits, np.ndarray) and isinstance(got.tree.parent, np.ndarray)
        _check(got, want, mode, ('numpy', mode))
        acts = gogame.uct_actions(mc.to_dev(roots), T, K, **kw, **mk)
        assert np.array_equal(mc.to_np(acts), mc.most_visited(want)), mode
        assert np.array_equal(gogame.uct_actions(np.array(roots), T, K, **kw, **mk), mc.most_visited(want)), mode
        root_keys, tree_keys = ml.keys(mode)
        for r in (0, 2):
            one = dict(mk)
            if 'last_actions' in one:
                one['last_actions'] = int(one['last_actions'][r])
            got = gogame.uct(mc.to_dev(roots[r]), T, K, first_root=r, tree=True, **kw, **one)
            for k in root_keys:
                assert np.array_equal(mc.to_np(getattr(got, k)), want[k][r]), (mode, r, k)
            for k in tree_keys:
                assert np.array_equal(mc.to_np(getattr(got.tree, k)), want['tree'][k][r]), (mode, r, k)
    empty = gogame.batch_uct(torch.zeros((0, 6, N, N), dtype=torch.uint8, device='cuda'), 3, 2, leaves=4, tree=True)
    assert tuple(empty.tree.parent.shape) == (0, 13) and tuple(empty.visits.shape) == (0, N * N + 1)


# ---------------------------------------------------------------- the entry points on the test's own buffers
TAIL = 256        # bytes of 0x5A behind every buffer


class Bufs:
    """Device buffers with a sentinel tail each."""

    def __init__(self):
        self.raw = {}

    def new(self, name, shape, dtype, value=None):
        es = torch.empty(0, dtype=dtype).element_size()
        n = int(np.prod(shape)) * es
        raw = torch.full((n + TAIL,), 0x5A, dtype=torch.uint8, device='cuda')
        self.raw[name] = (raw, n)
        view = raw[:n].view(dtype).view(tuple(shape))
        if value is not None:
            view.copy_(value)
        return view

    def broken(self):
        return [name for name, (raw, n) in self.raw.items() if not bool((raw[n:] == 0x5A).all())]


def _tree_buffers(new, R, N, C, rows, rave):
    W, A = 5 * N + 1, N * N + 1
    i32, i64 = torch.int32, torch.int64
    b = {'boards': new('boards', (R, C + 1, W), i32), 'child': new('child', (R, C + 1, A), i32), 'links': new('links', (R, C + 1, 2), i32),
         'stats': new('stats', (R, C + 1, 4), i32), 'nodes': new('nodes', (R,), i32), 'virt': new('virt', (R, C + 1), i32),
         'leaf': new('leaf', (rows, W), i32), 'move': new('move', (rows,), i32), 'leaf_id': new('leaf_id', (rows,), i32),
         'totals': new('totals', (R, 2), i64)}
    b['virt'].zero_()
    b['totals'].zero_()
    if rave:
        b['node_amaf'] = new('node_amaf', (R, C + 1, N * N, 2), i32)
        b['node_amaf'].zero_()
    return b


def _calls(b, R, N, C, L, K, c, mode, log_table, counts, sums, amaf, weights, one_leaf=False):
    """The argument tuples of the round's calls on the buffers b -> (select, expand or None, backup): the _leaves entry points, or
    with one_leaf their namesakes - the same lists without L and virt."""
    s = _stream()
    lf, lv, vt = ('', (), ()) if one_leaf else ('_leaves', (L,), (b['virt'],))
    if mode == 'plain':
        select = ('gg_uct_select' + lf, R, N, C, *lv, K, c, log_table, b['boards'], b['child'], b['links'], b['stats'], b['nodes'], *vt,
                  b['leaf'], b['move'], b['leaf_id'], s)
        backup = ('gg_uct_backup' + lf, R, N, C, *lv, K, counts, sums, b['totals'], b['boards'], b['links'], b['stats'], *vt, b['leaf'],
                  b['move'], b['leaf_id'], s)
        return select, None, backup
    select = ('gg_uct_select' + lf + '_rave', R, N, C, *lv, K, c, ml.EQUIV, ml.FPU, log_table, b['boards'], b['child'], b['links'],
              b['stats'], b['node_amaf'], b['nodes'], *vt, b['leaf'], b['move'], b['leaf_id'], s)
    backup = ('gg_uct_backup' + lf + '_rave', R, N, C, *lv, K, counts, sums, amaf, b['totals'], b['boards'], b['links'], b['stats'],
              b['node_amaf'], *vt, b['leaf'], b['move'], b['leaf_id'], s)
    expand = None
    if mode == 'prior':
        expand = ('gg_uct_prior_expand' + lf, R, N, C, *lv, weights, b['leaf'], b['move'], b['leaf_id'], b['node_amaf'], s)
    return select, expand, backup


def _path_counts(links, leaf_id, R, C, L):
    """int [R, C + 1]: per node the rows of the round whose path goes through it."""
    want = np.zeros((R, C + 1), np.int64)
    for r in range(R):
        for j in range(L):
            y = int(leaf_id[r * L + j])
            while y >= 0:
                want[r, y] += 1
                y = int(links[r, y, 0])
    return want


def _direct(roots, T, L, K, c, mode, seed, cap, komi, C=None, first_root=0, S=16, chunk=32):
    """The search through the entry points, as gogame._run_uct queues it, on buffers with sentinel tails; between the select and
    the backup of every round virt is the round's path counts and the empty rows hold the root's board, -1 and -1; after the
    backup every v is 0.  -> dict of NumPy arrays: child, links, stats, nodes, totals (node_amaf)."""
    from gymgo_amd import _lib, gogame
    R, N = roots.shape[0], roots.shape[-1]
    C = T * L if C is None else C
    rows, W = R * L, 5 * N + 1
    rave, prior = ml.mode_args(mode, R, N)
    dev = mc.to_dev(roots)
    tr = gogame.batch_track(dev)
    bufs = Bufs()
    b = _tree_buffers(bufs.new, R, N, C, rows, rave is not None)
    log_table = bufs.new('log_table', (C + 1,), torch.float64, torch.from_numpy(mc.log_table(C, K)).cuda())
    pbufs = gogame._playout_buffers(rows, S, N, 'cuda')
    abufs = gogame._amaf_buffers(rows, S, N, chunk, 'cuda') if rave is not None else None
    weights = _i32([x for p in prior[0] for x in p]) if prior is not None else None
    select, expand, backup = _calls(b, R, N, C, L, K, c, mode, log_table, pbufs[5], pbufs[6], None if abufs is None else abufs[3], weights)
    s = _stream()
    _lib.call('gg_uct_begin', tr, R, N, C, K, b['boards'], b['child'], b['links'], b['stats'], b['nodes'], s)
    if prior is not None:
        _lib.call('gg_uct_prior_begin', tr, _i32(prior[1]), R, N, C, weights, b['node_amaf'], s)
    for t in range(T):
        _lib.call(*select)
        leaf_id, move = b['leaf_id'].cpu().numpy(), b['move'].cpu().numpy()
        assert ((leaf_id >= -1) & (leaf_id <= C)).all() and (b['nodes'].cpu().numpy() <= C + 1).all(), (mode, t)
        assert np.array_equal(b['virt'].cpu().numpy(), _path_counts(b['links'].cpu().numpy(), leaf_id, R, C, L)), (mode, t, 'virt')
        empty = np.flatnonzero(leaf_id < 0)
        assert (move[empty] == -1).all(), (mode, t)
        for row in empty:
            assert torch.equal(b['leaf'][row], tr[row // L]), (mode, t, row)
        _lib.call('gg_batch_play_moves_tracked', b['leaf'], b['move'], None, rows, N, 1, s)
        if expand is not None:
            _lib.call(*expand)
        gogame._run_playouts(b['leaf'], rows, N, K, cap, komi, gogame._uct_seed(seed, t), first_root * L, False, S, chunk, dev.device, pbufs,
                             0, amaf=abufs)
        _lib.call(*backup)
        assert not bool(b['virt'].any()), (mode, t, 'virt after the backup')
    torch.cuda.synchronize()
    assert bufs.broken() == [], mode
    assert bool((dev == mc.to_dev(roots)).all())
    return {k: v.cpu().numpy() for k, v in b.items() if k in ('child', 'links', 'stats', 'nodes', 'totals', 'node_amaf')}


def _check_tree(got, want, mode, tag):
    t = want['tree']
    pairs = [('nodes', want['nodes']), ('child', t['child']), ('links', np.stack([t['parent'], t['action']], axis=-1)),
             ('stats', np.stack([t[k] for k in ('visits', 'black_wins', 'white_wins', 'draws')], axis=-1)),
             ('totals', np.stack([want['unfinished'], want['plies_sum']], axis=-1))]
    if mode != 'plain':
        pairs.append(('node_amaf', t['node_amaf']))
    for k, w in pairs:
        assert got[k].shape == w.shape, (tag, k, got[k].shape, w.shape)
        assert np.array_equal(got[k], w), (tag, k, np.argwhere(got[k] != w)[:6].tolist())


@pytest.mark.parametrize('mode', ml.MODES)
def test_entry_points_virt_empty_rows_and_sentinels(mode):
    for N, L in ((2, 8), (5, 4), (19, 4)):
        T, K, cap, _ = ml.size_shape(N)
        roots, want = ml.size_case(N, mode, L)
        got = _direct(roots, T, L, K, ml.size_c(mode), mode, ml.size_seed(N), cap, ml.KOMI)
        _check_tree(got, want, mode, (N, mode, L))
    roots, want = ml.ended_case(mode, 8)
    got = _direct(roots, ml.ENDED_T, 8, ml.ENDED_K, 0.3, mode, 77, 64, ml.KOMI)
    _check_tree(got, want, mode, ('ended', mode))


@pytest.mark.parametrize('mode', ml.MODES)
def test_a_select_past_capacity_writes_nothing_beyond_a_tree(mode):
    """Four rounds of four slots on trees with room for nine leaves: once a tree is full its slots evaluate the node they stand at,
    move = -1, and gg_uct_prior_expand_leaves leaves every pair as it is."""
    roots, want = ml.past_capacity_case(mode)
    assert mode == 'prior' or (want['nodes'][:2] == ml.PAST_C + 1).all()
    got = _direct(roots, ml.PAST_T, ml.PAST_L, ml.PAST_K, ml.size_c(mode), mode, 13, 64, ml.KOMI, C=ml.PAST_C)
    _check_tree(got, want, mode, ('past capacity', mode))


@pytest.mark.parametrize('mode', ml.MODES)
@pytest.mark.parametrize('N', (2, 9, 19))
def test_one_leaf_and_leaves_entry_points_agree_launch_for_launch(N, mode):
    """The two instantiations of the one kernel body, launch for launch: side A through gg_uct_select[_rave] ->
    gg_batch_play_moves_tracked -> (gg_uct_prior_expand) -> gg_uct_backup[_rave], side B through the _leaves entry points with
    L = 1 and a virt buffer, each on buffers of its own with sentinel tails.  Trees of 7 nodes, K = 2, eight rounds - the last two
    find no room in a tree that grew in every round before (at 9x9 and 19x19 there is one in every mode; on 2x2 a walk may end in a
    finished game, which adds no node, so a tree may stay below its capacity there).  The counts, sums and AMAF rows of a backup are the test's own numbers, the same on both sides and others in
    every round: no playout runs.  After every select and after every backup the tree and the round's rows are equal byte for byte;
    virt is the round's path counts in between and 0 after the backup."""
    from gymgo_amd import _lib, gogame
    roots = cs.stack(N, ('late0', 'mid0', 'empty', 'ended'))
    R, C, K, T, P = len(roots), 6, 2, 8, N * N
    rave, prior = ml.mode_args(mode, R, N)
    tr = gogame.batch_track(mc.to_dev(roots))
    weights = _i32([x for p in prior[0] for x in p]) if prior is not None else None
    counts = torch.zeros((R, 4), dtype=torch.int32, device='cuda')
    sums = torch.zeros((R, 2), dtype=torch.int64, device='cuda')
    amaf = torch.zeros((R, 2, 3, N, N), dtype=torch.int32, device='cuda') if rave is not None else None
    s = _stream()
    sides = []
    for one_leaf in (True, False):
        bufs = Bufs()
        b = _tree_buffers(bufs.new, R, N, C, R, rave is not None)
        log_table = bufs.new('log_table', (C + 1,), torch.float64, torch.from_numpy(mc.log_table(C, K)).cuda())
        _lib.call('gg_uct_begin', tr, R, N, C, K, b['boards'], b['child'], b['links'], b['stats'], b['nodes'], s)
        if prior is not None:
            _lib.call('gg_uct_prior_begin', tr, _i32(prior[1]), R, N, C, weights, b['node_amaf'], s)
        sides.append((bufs, b, _calls(b, R, N, C, 1, K, ml.size_c(mode), mode, log_table, counts, sums, amaf, weights, one_leaf)))
    names = ('child', 'links', 'stats', 'nodes', 'leaf', 'move', 'leaf_id') + (('node_amaf',) if rave is not None else ())

    def same(tag):
        (_, a, _), (_, b, _) = sides
        for k in names:
            assert torch.equal(a[k], b[k]), (N, mode, tag, k)
        assert (a['nodes'] <= C + 1).all() and (b['nodes'] <= C + 1).all(), (N, mode, tag)
        for bufs, _, _ in sides:
            assert bufs.broken() == [], (N, mode, tag)

    virt = sides[1][1]['virt']
    rng = np.random.RandomState(100 * N + len(mode))
    same('begin')
    met_full = False
    for t in range(T):
        full = sides[0][1]['nodes'].cpu().numpy() == C + 1                        # before the select
        for _, b, (select, _, _) in sides:
            _lib.call(*select)
        same((t, 'select'))
        links, leaf_id = sides[1][1]['links'].cpu().numpy(), sides[1][1]['leaf_id'].cpu().numpy()
        assert ((leaf_id >= 0) & (leaf_id <= C)).all(), (N, mode, t)            # L = 1: no collision, no empty slot
        assert np.array_equal(virt.cpu().numpy(), _path_counts(links, leaf_id, R, C, 1)), (N, mode, t, 'virt')
        if t >= C:                                                                # a tree that is full: nothing is added
            assert (sides[0][1]['move'].cpu().numpy()[full] == -1).all(), (N, mode, t)
            assert (sides[0][1]['nodes'].cpu().numpy()[full] == C + 1).all(), (N, mode, t)
            met_full |= bool(full.any())
        for _, b, (_, expand, _) in sides:
            _lib.call('gg_batch_play_moves_tracked', b['leaf'], b['move'], None, R, N, 1, s)
            if expand is not None:
                _lib.call(*expand)
        # the round's results: K playouts per row split into black wins, white wins and draws, first plays of at most K a point
        bw = rng.randint(0, K + 1, R)
        ww = rng.randint(0, K + 1 - bw)
        counts.copy_(_i32(np.stack([bw, ww, K - bw - ww, rng.randint(0, 2, R)], axis=-1)))
        sums.copy_(torch.from_numpy(rng.randint(0, 1000, (R, 2)).astype(np.int64)).cuda())
        if amaf is not None:
            e0 = rng.randint(0, K + 1, (R, 2, N, N))
            e1 = rng.randint(0, e0 + 1)
            amaf.copy_(_i32(np.stack([e0, e1, rng.randint(0, e0 - e1 + 1)], axis=2)))
        for _, b, (_, _, backup) in sides:
            _lib.call(*backup)
        same((t, 'backup'))
        assert torch.equal(sides[0][1]['totals'], sides[1][1]['totals']), (N, mode, t)
        assert not bool(virt.any()), (N, mode, t, 'virt after the backup')
    nodes = sides[0][1]['nodes'].cpu().numpy()
    assert (met_full or N == 2) and nodes[-1] == 1, (N, mode, nodes)             # full trees; the ended root stays alone


# ---------------------------------------------------------------- guards
def _arena(specs, k):
    """An arena with one view per (name, shape, dtype) of specs, buffer j at the (k + j)-th residue its element size allows."""
    import guard_arena as ga
    arena = ga.Arena(sum(ga.footprint(shape, dtype) for _, shape, dtype in specs) + 64, 'cuda')
    views = {}
    for j, (name, shape, dtype) in enumerate(specs):
        res = ga.residues(dtype)
        views[name] = arena.take(name, shape, dtype, res[(k + j) % len(res)])
    return arena, views


def _readonly(arena, names):
    for name in arena.regions:
        arena.set_readonly(name, name in names)


@pytest.mark.parametrize('mode', ('plain', 'prior'))
@pytest.mark.parametrize('N', (2, 9, 19))
def test_guards_every_entry_point_at_every_start_residue(N, mode):
    """Round 2 of a search of three roots and three slots, every buffer a view of one arena between guards: each of the (three
    plain, five RAVE and prior) calls writes its outputs as on plain tensors, and nothing else - not the guards, not what it takes
    as const."""
    from gymgo_amd import _lib, gogame
    roots = cs.stack(N, ('late0', 'mid0', 'ended'))
    R, L, T, K, cap, S = len(roots), 3, 2, 2, 32, 8
    C, rows, W, P = T * L, R * L, 5 * N + 1, N * N
    rave, prior = ml.mode_args(mode, R, N)
    tr = gogame.batch_track(mc.to_dev(roots))
    i32, i64 = torch.int32, torch.int64
    log_np = torch.from_numpy(mc.log_table(C, K)).cuda()
    weights0 = _i32([x for p in prior[0] for x in p]) if prior is not None else None
    pbufs = gogame._playout_buffers(rows, S, N, 'cuda')
    abufs = gogame._amaf_buffers(rows, S, N, 32, 'cuda') if rave is not None else None
    # the reference: round 1 and round 2 on plain tensors, the state in front of every call of round 2 kept
    plain = Bufs()
    b = _tree_buffers(plain.new, R, N, C, rows, rave is not None)
    amaf0 = None if abufs is None else abufs[3]
    select, expand, backup = _calls(b, R, N, C, L, K, 0.4, mode, log_np, pbufs[5], pbufs[6], amaf0, weights0)
    s = _stream()
    _lib.call('gg_uct_begin', tr, R, N, C, K, b['boards'], b['child'], b['links'], b['stats'], b['nodes'], s)
    if prior is not None:
        _lib.call('gg_uct_prior_begin', tr, _i32(prior[1]), R, N, C, weights0, b['node_amaf'], s)
    keep = lambda: {k: v.clone() for k, v in b.items()}
    states = {}
    for t in range(T):
        states['select'] = keep()
        _lib.call(*select)
        _lib.call('gg_batch_play_moves_tracked', b['leaf'], b['move'], None, rows, N, 1, s)
        states['played'] = keep()
        if expand is not None:
            _lib.call(*expand)
        states['expanded'] = keep()
        gogame._run_playouts(b['leaf'], rows, N, K, cap, ml.KOMI, gogame._uct_seed(3, t), 0, False, S, 32, tr.device, pbufs, 0, amaf=abufs)
        _lib.call(*backup)
        states['end'] = keep()
    counts, sums = pbufs[5].clone(), pbufs[6].clone()          # (of round 2, as amaf0)
    assert bool((states['end']['leaf_id'] >= 0).any()) and bool((states['end']['nodes'] > 1).any())
    assert mode == 'plain' or not torch.equal(states['played']['node_amaf'], states['expanded']['node_amaf'])
    specs = [('boards', (R, C + 1, W), i32), ('child', (R, C + 1, N * N + 1), i32), ('links', (R, C + 1, 2), i32), ('stats', (R, C + 1, 4), i32),
             ('nodes', (R,), i32), ('virt', (R, C + 1), i32), ('leaf', (rows, W), i32), ('move', (rows,), i32), ('leaf_id', (rows,), i32),
             ('totals', (R, 2), i64), ('log_table', (C + 1,), torch.float64), ('counts', (rows, 4), i32), ('sums', (rows, 2), i64)]
    if rave is not None:
        specs += [('node_amaf', (R, C + 1, P, 2), i32), ('amaf', (rows, 2, 3, N, N), i32), ('weights', (12,), i32)]
    # (step, the state in front of it, what it must leave as it is, the state behind it - behind the select: with its moves played)
    steps = [('select', 'select', ('boards', 'log_table', 'node_amaf', 'totals', 'counts', 'sums', 'amaf', 'weights'), 'played')]
    if mode == 'prior':
        steps.append(('expand', 'played', tuple(n for n, _, _ in specs if n != 'node_amaf'), 'expanded'))
    steps.append(('backup', 'expanded', ('child', 'links', 'nodes', 'leaf', 'move', 'leaf_id', 'log_table', 'counts', 'sums', 'amaf', 'weights'),
                  'end'))
    for k in range(16):
        arena, v = _arena(specs, k)
        v['log_table'].copy_(log_np)
        v['counts'].copy_(counts)
        v['sums'].copy_(sums)
        if rave is not None:
            v['amaf'].copy_(amaf0)
            v['weights'].copy_(weights0)
        calls = dict(zip(('select', 'expand', 'backup'),
                         _calls(v, R, N, C, L, K, 0.4, mode, v['log_table'], v['counts'], v['sums'], v.get('amaf'), v.get('weights'))))
        for step, before, const, behind in steps:
            for name, t0 in states[before].items():
                v[name].copy_(t0)
            _readonly(arena, const)
            arena.snapshot()
            _lib.call(*calls[step])
            assert arena.violations() == [], (N, mode, k, step)
            if step == 'select':
                _lib.call('gg_batch_play_moves_tracked', v['leaf'], v['move'], None, rows, N, 1, s)
            for name, t1 in states[behind].items():
                assert torch.equal(v[name], t1), (N, mode, k, step, name)


# ---------------------------------------------------------------- one compute unit: later trips, and both playout kernel families
ONE_CU = r'''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
from gymgo_amd import _lib, gogame
import mc_cases as cs
import mc_expect as mc
import mc_policy_expect as mp
import mc_tactics_expect as mt
import mc_uct_leaves_expect as ml
assert _lib.lib().gg_device_cus() == 1


def check(got, want, mode, tag):
    root_keys, tree_keys = ml.keys(mode)
    mc.check(got, want, root_keys, tag)
    mc.check(got.tree, want['tree'], tree_keys, (tag, 'tree'))


def mode_kw(mode, R, N):
    rave, prior = ml.mode_args(mode, R, N)
    kw = {}
    if rave is not None:
        kw.update(rave_equiv=rave[0], fpu=rave[1])
    if prior is not None:
        kw.update(prior=gogame.UctPrior(*prior[0]), last_actions=prior[1])
    return kw


# one compute unit: the tree kernels run 32 workgroups of four waves, 128 roots a trip; the prior kernel 64 workgroups of four
# boards, 256 rows a trip.  150 roots x 3 slots: the second trip of the one, the second of the other
N, R, T, L, K = 5, 150, 2, 3, 1
base = cs.stack(N)
roots = base[(7 * np.arange(R)) %% len(base)]
for mode in ml.MODES:
    rave, prior = ml.mode_args(mode, R, N)
    want = ml.expected_uct_leaves(roots, T, L, K, c=ml.size_c(mode), rave=rave, prior=prior, max_plies=64, komi=ml.KOMI, base_seed=8)
    got = gogame.batch_uct(torch.from_numpy(roots).cuda(), T, K, c=ml.size_c(mode), max_plies=64, komi=ml.KOMI, seed=8, leaves=L, tree=True,
                           **mode_kw(mode, R, N))
    check(got, want, mode, ('trips', mode))
# 9x9, 2 roots x 32 slots x 4 playouts = 256 jobs: on 256 slots the thirty-two-board kernel runs the leaf playouts, on 48 the
# one-row-per-lane kernel - every playout policy on both, plain (the policy kernels) and RAVE (their move-log variants)
N, T, L, K = 9, 2, 32, 4
roots = cs.stack(N, ('mid0', 'mid1'))
dev = torch.from_numpy(roots).cuda()
rollouts = {'uniform': None, 'no_eye_fill': mp.policy_rollout, 'tactical': mt.tactical_rollout}
for policy, mode in (('uniform', 'plain'), ('uniform', 'rave'), ('no_eye_fill', 'plain'), ('no_eye_fill', 'rave'), ('tactical', 'plain'),
                     ('tactical', 'rave')):
    rave, _ = ml.mode_args(mode, 2, N)
    want = ml.expected_uct_leaves(roots, T, L, K, c=ml.size_c(mode), rave=rave, max_plies=32, komi=7.5, base_seed=19,
                                  policy=list(rollouts).index(policy), rollout=rollouts[policy])
    assert want['live'].min() >= 24
    for S in (256, 48):
        got = gogame.batch_uct(dev, T, K, c=ml.size_c(mode), max_plies=32, komi=7.5, seed=19, leaves=L, tree=True, slots=S, policy=policy,
                               **mode_kw(mode, 2, N))
        check(got, want, mode, (policy, mode, S))
torch.cuda.synchronize()
print('UCT LEAVES ONE CU OK')
''' % (ROOT, os.path.join(ROOT, 'tests'))


def test_one_compute_unit_later_trips_and_both_kernel_families():
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '1'
    p = subprocess.run([sys.executable, '-c', ONE_CU], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert 'UCT LEAVES ONE CU OK' in p.stdout
