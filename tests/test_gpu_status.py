"""-m gpu: stone status and the final score from playout ownership (k_status, gg_status.h; gogame.batch_stone_status /
batch_stone_status_tracked / stone_status / batch_final_score / final_score), every byte equal to tests/status_expect.py - at
EVERY board size from 2 to 19 on the three sets of tests/plane_cases.py with generated ownership counts (chains on and one
count below either inequality), with `side` absent, constant and mixed, in all eight views, at three thresholds; one chain of
360 stones at 2^20 playouts; the empty board, a full-but-one board and the corridor boards; sub-batches between sentinels;
both entry points inside a guarded arena; later trips of the grid-stride loop; and the final score of real playouts against
the CPU replay.  tests/test_status_host.py holds what this file relies on."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import area_expect as ae
import mc_expect as mc
import mc_policy_expect as mp
import plane_cases as pc
import status_expect as se

B = pc.B
SENTINEL = 0xA5
B_TRIPS = 533
TRIP_SIZES = (9, 13, 19)
ARENA_SIZES = (2, 9, 13, 19)


def same(got, want, tag=''):
    got = mc.to_np(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want), (tag, np.argwhere(got != want)[:8])


def dtype_of(N):
    import test_gpu_plane_sizes as tps
    return tps.dtype_of(N)


def mixed(n):
    import test_gpu_life as tgl
    return tgl.mixed(n)


def forms(gogame, st):
    return (('bytes', st, gogame.batch_stone_status), ('tracked', gogame.batch_track(st), gogame.batch_stone_status_tracked))


def check_set(N, c, tag, orient=None):
    """Every `side` form of one set, byte planes and tracked, plain or in the views `orient` (want = the turned expectation;
    the ownership counts stay in the stored frame, the counts do not turn)."""
    import torch
    from gymgo_amd import gogame
    n = len(c.states)
    st = mc.to_dev(c.states.copy())         # (the cached arrays are read-only)
    own = mc.to_dev(c.own.copy())
    before = own.clone()
    thr = (c.num, c.den)
    turn = (lambda p: p) if orient is None else (lambda p: pc.turned(p, orient))
    kw = {} if orient is None else {'orient': torch.from_numpy(orient).cuda()}
    side = ae.mixed_side(n)
    want_mixed = np.where(side[:, None, None, None] != 0, c.white, c.black)
    counts_mixed = np.where(side[:, None] != 0, c.counts_white, c.counts_black)
    for name, x, fn in forms(gogame, st):
        for what, s, planes, counts in (('own turn', None, c.planes, c.counts), ('black', np.zeros(n, np.uint8), c.black, c.counts_black),
                                        ('white', np.ones(n, np.uint8), c.white, c.counts_white), ('mixed', side, want_mixed, counts_mixed)):
            got, cnt = fn(x, own, c.K, thr, side=None if s is None else torch.from_numpy(s).cuda(), counts=True, **kw)
            same(got, turn(planes), tag + (name, what))
            same(cnt, counts, tag + (name, what, 'counts'))
            same(fn(x, own, c.K, thr, side=s, **kw), turn(planes), tag + (name, what, 'without counts, side as an array'))
        got, cnt = fn(x, own, c.K, thr, dtype=dtype_of(N), side=side.astype(bool), counts=True, **kw)
        assert got.dtype == dtype_of(N)
        same(got.to(torch.uint8), turn(want_mixed), tag + (name, 'dtype'))
        same(cnt, counts_mixed, tag + (name, 'dtype, counts'))
    assert torch.equal(own, before), tag
    if orient is not None:                   # ... and the plain call on the turned boards with the turned ownership counts
        turned = gogame.batch_symmetry(st, kw['orient'] & 7)
        own_t = mc.to_dev(pc.turned(c.own, orient))
        for name, x, fn in forms(gogame, turned):
            got, cnt = fn(x, own_t, c.K, thr, counts=True)
            same(got, turn(c.planes), tag + (name, 'the turned position'))
            same(cnt, c.counts, tag + (name, 'the turned position, counts'))


@pytest.mark.gpu
@pytest.mark.parametrize('N', pc.SIZES)
def test_plain_calls_byte_planes_and_tracked(N):
    for thr in se.THRESHOLDS:
        for kind in pc.SETS:
            check_set(N, se.case(N, kind, thr), (N, kind, thr))


@pytest.mark.gpu
@pytest.mark.parametrize('N', pc.SIZES)
def test_oriented_calls_byte_planes_and_tracked(N):
    orient = mixed(B)                        # all eight views, with the negative and the large words
    assert set(orient & 7) == set(range(8)) and orient.min() < 0 and orient.max() > 7
    for thr in se.THRESHOLDS:
        for kind in pc.SETS:
            check_set(N, se.case(N, kind, thr), (N, kind, thr, 'oriented'), orient)


@pytest.mark.gpu
@pytest.mark.parametrize('num', (1024, 1000))
def test_large_value_case(num):
    """One chain of 360 stones at K = 2^20, den = 1024, D on the inequality and one count below it: sums beyond 2^28, products
    beyond 2^32 (tests/test_status_host.py: a 32-bit product or a packed 16-bit sum gets it wrong)."""
    import torch
    from gymgo_amd import gogame
    c = se.large_case(num)
    st, own = mc.to_dev(c.states.copy()), mc.to_dev(c.own.copy())
    zero = np.zeros(4, np.uint8)
    for name, x, fn in forms(gogame, st):
        got, cnt = fn(x, own, c.K, (c.num, c.den), side=zero, counts=True)
        same(got, c.black, (num, name))
        same(cnt, c.counts_black, (num, name, 'counts'))
        dead = mc.to_np(got)[:, [1, 4]].sum(axis=(1, 2, 3))
        assert list(dead) == [360, 0, 360, 0], (num, name, dead)
        got, cnt = fn(x, own, c.K, (c.num, c.den), side=zero, counts=True, orient=np.array([5, 2, 7, 4]), dtype=torch.float32)
        same(got.to(torch.uint8), pc.turned(c.black, np.array([5, 2, 7, 4])), (num, name, 'oriented'))
        same(cnt, c.counts_black, (num, name, 'oriented, counts'))


def edge_boards(N):
    """The empty board, black's and white's full-but-one boards (a single chain with one liberty, the liberty in a corner and
    in the middle), with generated ownership counts at every threshold -> [(case-like namespace)]."""
    from types import SimpleNamespace
    s = np.zeros((5, 6, N, N), np.uint8)
    for i, (col, hole) in enumerate(((0, (0, 0)), (1, (N - 1, N - 1)), (0, (N // 2, N // 2)), (1, (0, N - 1)))):
        s[1 + i, col] = 1
        s[1 + i, col][hole] = 0
        s[1 + i, 2] = i % 2
    out = []
    for thr in se.THRESHOLDS:
        K = se.PLAYOUTS[thr]
        own, info = se.generated(s, K, thr[0], thr[1], seed=N)
        c = SimpleNamespace(states=s, own=own, K=K, num=thr[0], den=thr[1])
        c.black, c.counts_black = se.batch_status(s, own, K, thr[0], thr[1], side=0)
        c.white, c.counts_white = se.white_view(c.black, c.counts_black)
        white = s[:, 2, 0, 0] != 0
        c.planes, c.counts = np.where(white[:, None, None, None], c.white, c.black), np.where(white[:, None], c.counts_white, c.counts_black)
        out.append(c)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('N', pc.SIZES)
def test_empty_full_but_one_and_corridor_boards(N):
    for c in edge_boards(N):
        assert not c.black[0, :8].any() and c.black[0, 8].all()                   # the empty board: all neutral
        check_set(N, c, (N, 'edge', c.num, c.den))
        check_set(N, c, (N, 'edge', c.num, c.den, 'oriented'), mixed(5))
    c = se.case(N, 'corridor')
    if N >= 5:
        assert len(c.states) == 32
    if len(c.states):
        check_set(N, c, (N, 'corridor'))
        check_set(N, c, (N, 'corridor', 'oriented'), mixed(len(c.states)))


def room(lead, n, dt):
    """n elements of dt at `lead` elements into a sentinel-filled buffer, and whether everything around them is untouched."""
    import torch
    size = torch.empty(0, dtype=dt).element_size()
    raw = torch.full(((lead + n) * size + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
    return raw[lead * size:(lead + n) * size].view(dt), lambda: bool((raw[:lead * size] == SENTINEL).all()) and bool(
        (raw[(lead + n) * size:] == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize('N', pc.SIZES)
def test_sub_batches_between_sentinels(N):
    """A lone board and a wave that is not full, from three places of the batch, written through out= into a slice of a
    larger buffer at 1, 7 or 20 elements into it (out needs its element's alignment only), the counts into a slice of a larger
    int32 buffer.  Nothing before or behind either slice is written.  All four dtypes at every N."""
    import torch
    from gymgo_amd import gogame
    P = N * N
    for j, kind in enumerate(pc.SETS):
        c = se.case(N, kind)
        st, own = mc.to_dev(c.states.copy()), mc.to_dev(c.own.copy())
        tracked = gogame.batch_track(st)
        side = ae.mixed_side(B)
        want = np.where(side[:, None, None, None] != 0, c.white, c.black)
        want_counts = np.where(side[:, None] != 0, c.counts_white, c.counts_black)
        for nb in (1, 3):
            for k, first in enumerate((0, 7, B - nb)):
                lead, sl = (1, 7, 20)[k], slice(first, first + nb)
                for d, dt in enumerate((torch.uint8, torch.float16, torch.bfloat16, torch.float32)):
                    tag = (N, kind, dt, nb, first)
                    flat, untouched = room(lead, nb * 9 * P, dt)
                    cflat, cuntouched = room(1 + 2 * k, nb * 4, torch.int32)
                    out, cnt = flat.view(nb, 9, N, N), cflat.view(nb, 4)
                    fn, x = ((gogame.batch_stone_status, st), (gogame.batch_stone_status_tracked, tracked))[(k + d + j) % 2]
                    got, gc = fn(x[sl], own[sl], c.K, (c.num, c.den), dtype=dt, out=out, side=side[sl], counts=cnt)
                    assert got is out and gc is cnt
                    same(out.to(torch.uint8), want[sl], tag)
                    same(cnt, want_counts[sl], tag + ('counts',))
                    assert untouched() and cuntouched(), tag


# ---------------------------------------------------------------- a guarded arena
@pytest.mark.gpu
@pytest.mark.parametrize('N', ARENA_SIZES)
def test_both_entry_points_inside_a_guarded_arena(N):
    """Every buffer of a call as a view of ONE tensor between guards (tests/guard_arena.py), the boards at every start residue
    mod 16 and the other buffers at every residue their element allows: no byte outside a buffer is written, no input - own
    among them - changes, and the result is the plain call's."""
    import torch
    import guard_arena as ga
    from gymgo_amd import gogame, _lib
    nb = 5
    c = se.case(N, 'random')
    states, own = c.states[:nb], c.own[:nb]
    orient, side = mixed(nb), ae.mixed_side(nb)
    want = pc.turned(np.where(side[:, None, None, None] != 0, c.white[:nb], c.black[:nb]), orient)
    want_counts = np.where(side[:, None] != 0, c.counts_white[:nb], c.counts_black[:nb])
    tracked = mc.to_np(gogame.batch_track(mc.to_dev(states.copy())))
    dtypes = (torch.uint8, torch.float16, torch.bfloat16, torch.float32)
    for r in range(16):
        for fn, boards in (('gg_batch_status', states), ('gg_batch_status_tracked', tracked)):
            dt = dtypes[(r + (fn[-1] == 'd')) % 4]
            es = ga.element_size(dt)
            shapes = (('boards', boards.shape, torch.uint8 if boards.dtype == np.uint8 else torch.int32), ('orient', (nb,), torch.int32),
                      ('side', (nb,), torch.uint8), ('own', own.shape, torch.int32), ('out', (nb, 9, N, N), dt), ('counts', (nb, 4), torch.int32))
            arena = ga.Arena(sum(ga.footprint(s, t) for _, s, t in shapes) + 64, 'cuda')
            v = {}
            for k, (name, shape, t) in enumerate(shapes):
                step = ga.element_size(t)
                v[name] = arena.take(name, shape, t, ((r + 3 * k) * step) % 16, readonly=name not in ('out', 'counts'))
            v['boards'].copy_(torch.from_numpy(boards.copy()))
            v['orient'].copy_(torch.from_numpy(orient.copy()))
            v['side'].copy_(torch.from_numpy(side.copy()))
            v['own'].copy_(torch.from_numpy(own.copy()))
            arena.snapshot()
            _lib.call(fn, v['boards'], v['orient'], v['side'], v['own'], c.K, c.num, c.den, v['out'], v['counts'],
                      gogame.FEATURE_DTYPES[dt], nb, N, _lib.stream_ptr(v['out'].device))
            torch.cuda.synchronize()
            assert arena.violations() == [], (N, r, fn, arena.violations())
            same(v['out'].to(torch.uint8), want, (N, r, fn))
            same(v['counts'], want_counts, (N, r, fn, 'counts'))
            same(v['own'], own, (N, r, fn, 'own'))


# ---------------------------------------------------------------- later trips of the grid-stride loop
def pool_data(N):
    """The pool of 63 boards - policy ++ clean ++ random - with its ownership counts, its expectation from both sides, a mixed
    `side` vector and the views mixed(21)[i mod 21] of pool board i."""
    kinds = ('policy', 'clean', 'random')
    cat = lambda f: np.concatenate([getattr(se.case(N, k), f) for k in kinds])
    d = {f: cat(f) for f in ('states', 'own', 'planes', 'black', 'white', 'counts', 'counts_black', 'counts_white')}
    d['orient'] = np.tile(mixed(B), 3)
    d['side'] = ae.mixed_side(63)
    c = se.case(N, 'policy')
    d['scalars'] = np.array([c.K, c.num, c.den])
    assert len(d['states']) == 63
    return d


def _trips_child(N, path):
    import torch
    from gymgo_amd import gogame, _lib
    assert _lib.lib().gg_device_cus() == 1
    d = dict(np.load(path))
    K, num, den = (int(x) for x in d['scalars'])
    i63 = (5 * np.arange(B_TRIPS)) % 63
    st = torch.from_numpy(d['states'][i63]).cuda()
    own = torch.from_numpy(d['own'][i63]).cuda()
    orient, side = d['orient'][i63], d['side'][i63]
    mix = lambda a, b: np.where(side.reshape((-1,) + (1,) * (d[a].ndim - 1)) != 0, d[a][i63], d[b][i63])
    cases = (('own turn', None, d['planes'][i63], d['counts'][i63]), ('mixed', side, mix('white', 'black'), mix('counts_white', 'counts_black')))
    for form, x, fn in (('bytes', st, gogame.batch_stone_status), ('tracked', gogame.batch_track(st), gogame.batch_stone_status_tracked)):
        for v, o in enumerate((None, orient)):
            for w, (what, s, planes, counts) in enumerate(cases):
                tag = (N, form, 'plain' if o is None else 'oriented', what)
                want = planes if o is None else pc.turned(planes, o)
                flat, untouched = room(1 + 2 * v + 4 * w, want.size, torch.uint8)
                cflat, cuntouched = room(3 + v, counts.size, torch.int32)
                out, cnt = flat.view(want.shape), cflat.view(counts.shape)
                got, gc = fn(x, own, K, (num, den), out=out, orient=o, side=s, counts=cnt)
                assert got is out and gc is cnt, tag
                same(out, want, tag)
                same(cnt, counts, tag + ('counts',))
                assert untouched() and cuntouched(), tag
                # ... and against the call in chunks of 64 boards (one trip each)
                for a in range(0, B_TRIPS, 64):
                    sl = slice(a, min(a + 64, B_TRIPS))
                    part, pc_ = fn(x[sl], own[sl], K, (num, den), orient=None if o is None else o[sl], side=None if s is None else s[sl],
                                   counts=True)
                    assert torch.equal(part, out[sl]) and torch.equal(pc_, cnt[sl]), tag + (a,)
    torch.cuda.synchronize()
    print('TRIPS ' + json.dumps({'N': N, 'ok': True}))


@pytest.mark.gpu
@pytest.mark.parametrize('N', TRIP_SIZES)
def test_later_trips_of_the_grid_stride_loop(N, tmp_path):
    """A fresh child process with the library sized for ONE compute unit (a grid of 64 workgroups) and 533 boards: 134 groups
    of four - three trips - or 267 groups of two - five trips -, the last group one board."""
    nbw = 4 if N <= 13 else 2
    groups = (B_TRIPS + nbw - 1) // nbw
    assert groups == (134 if nbw == 4 else 267) and B_TRIPS % nbw == 1
    path = str(tmp_path / 'pool.npz')
    np.savez(path, **pool_data(N))
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '1'
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(N), path], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith('TRIPS ')][-1]
    assert json.loads(line[len('TRIPS '):]) == {'N': N, 'ok': True}


# ---------------------------------------------------------------- the final score of real playouts
FINAL_K = 16


def final_roots(name):
    """(roots uint8 [R, 6, N, N], max_plies or None)"""
    if name == 'crafted7':
        return se.crafted_roots()[0][None], None
    if name == 'lone5':
        return se.crafted_roots()[1][None], None
    N = int(name)
    return mc.make_roots(N, 5, 40 + N, max_ply=200 if N == 19 else 40, step=56 if N == 19 else 8), (256 if N == 19 else None)


def check_final(got, want, po, tag):
    import torch
    from gymgo_amd import gogame
    assert isinstance(got, gogame.FinalScore) and isinstance(got.playouts, gogame.Playouts), tag
    for k, dt in (('black_area', np.int32), ('white_area', np.int32), ('margin', np.int32), ('winner', np.float64), ('owner', np.int8),
                  ('dead', np.uint8), ('unsettled', np.uint8)):
        g = mc.to_np(getattr(got, k))
        assert g.dtype == dt, (tag, k, g.dtype)
        same(g, want[k].astype(dt), tag + (k,))
    mc.check(got.playouts, po, mc.KEYS + ('ownership',), tag)


@pytest.mark.gpu
@pytest.mark.parametrize('policy', ('no_eye_fill', 'uniform'))
@pytest.mark.parametrize('name', ('crafted7', 'lone5', '5', '9', '19'))
def test_batch_final_score(name, policy):
    """Expectation: status_expect on expected_playouts(..., with_ownership=True); winner against batch_winning of the board
    with the dead stones removed; NumPy in / out and the single-state forms."""
    import torch
    from gymgo_amd import gogame
    roots, max_plies = final_roots(name)
    N = roots.shape[-1]
    komi = 0.5 if name in ('9', '19') else 0.0
    plies = max_plies if max_plies is not None else -(-8 * N * N // 32) * 32
    expected = mp.expected_playouts_policy if policy == 'no_eye_fill' else mc.expected_playouts
    po = expected(roots, FINAL_K, plies, komi=komi, with_ownership=True)
    want = se.final_score(roots, po['ownership'], FINAL_K, 2, 3, komi)
    kw = dict(komi=komi, policy=policy)
    if max_plies is not None:
        kw['max_plies'] = max_plies
    st = mc.to_dev(roots)
    got = gogame.batch_final_score(st, FINAL_K, **kw)
    check_final(got, want, po, (name, policy))
    assert torch.equal(got.margin, got.black_area - got.white_area)
    # the sign batch_winning gives for the board with the dead stones taken off
    rest = mc.to_dev(se.without_dead(roots, want['dead']))
    assert torch.equal(got.winner, gogame.batch_winning(rest, komi)), (name, policy)
    black, white = gogame.batch_areas(rest)
    assert torch.equal(black, got.black_area) and torch.equal(white, got.white_area)
    # another threshold: the status call on the same playouts
    t = se.final_score(roots, po['ownership'], FINAL_K, 1, 1, komi)
    same(gogame.batch_final_score(st, FINAL_K, threshold=(1, 1), **kw).dead, t['dead'], (name, policy, '(1, 1)'))
    # Playouts in place of their ownership; NumPy in gives NumPy out; the single-state forms
    planes, counts = gogame.batch_stone_status(st, got.playouts, FINAL_K, side=np.zeros(len(roots), np.uint8), counts=True)
    same(planes[:, 1] | planes[:, 4], want['dead'], (name, policy, 'from Playouts'))
    same(counts[:, 0], want['black_area'].astype(np.int32), (name, policy, 'from Playouts, counts'))
    got_np = gogame.batch_final_score(roots.copy(), FINAL_K, **kw)
    assert all(isinstance(x, np.ndarray) for x in got_np[:7]) and isinstance(got_np.playouts.ownership, np.ndarray)
    check_final(got_np, want, po, (name, policy, 'numpy'))
    one = gogame.final_score(st[-1], FINAL_K, first_root=len(roots) - 1, **kw)
    for k in ('black_area', 'white_area', 'margin', 'winner', 'owner', 'dead', 'unsettled'):
        same(getattr(one, k), np.asarray(want[k])[-1].astype(mc.to_np(getattr(one, k)).dtype), (name, policy, 'single', k))
    same(one.playouts.ownership, po['ownership'][-1], (name, policy, 'single, ownership'))
    p1, c1 = gogame.stone_status(st[-1], one.playouts, FINAL_K, side=0, counts=True)
    w1, wc1 = se.status_planes(roots[-1], po['ownership'][-1], FINAL_K, 2, 3, side=0)
    same(p1, w1, (name, policy, 'stone_status')), same(c1, wc1, (name, policy, 'stone_status counts'))
    p2 = gogame.stone_status(roots[-1].copy(), po['ownership'][-1], FINAL_K, dtype=torch.float32)
    assert isinstance(p2, np.ndarray) and p2.dtype == np.float32
    same(p2.astype(np.uint8), se.status_planes(roots[-1], po['ownership'][-1], FINAL_K, 2, 3)[0], (name, policy, 'stone_status numpy'))


@pytest.mark.gpu
def test_crafted_positions_on_the_device():
    """The 7x7 position at K = 64: exactly the two intruders are dead, nothing is unsettled, 22 / 21 and six neutral points
    (tests/test_status_host.py says why not 21 / 21 / 7); the lone stones of the 5x5 board are unsettled."""
    from gymgo_amd import gogame
    r7, r5 = se.crafted_roots()
    f = gogame.final_score(mc.to_dev(r7), 64, max_plies=392, chunk_plies=56)
    dead = mc.to_np(f.dead)
    assert dead.sum() == 2 and dead[2, 1] and dead[2, 5] and not mc.to_np(f.unsettled).any()
    assert (int(f.black_area), int(f.white_area), int(f.margin), float(f.winner)) == (22, 21, 1, 1.0)
    assert (mc.to_np(f.owner) == 0).sum() == 6
    f = gogame.final_score(mc.to_dev(r5), 64, max_plies=392, chunk_plies=56)
    assert mc.to_np(f.unsettled).sum() == 2 and not mc.to_np(f.dead).any()


if __name__ == '__main__':
    _trips_child(int(sys.argv[1]), sys.argv[2])
