"""-m gpu: the area ownership planes (k_area, gg_area.h; gogame.batch_area_planes / batch_area_planes_tracked / area_planes),
the ownership and score targets made from them (gogame.batch_ownership, selfplay_batch(ownership=True)) and the planes the
search hands out (PuctSearch(area=True)), every byte equal to tests/area_expect.py - at EVERY board size from 2 to 19 on the
three sets of tests/plane_cases.py, on the corridor boards (the deepest flood a board allows), with `side` absent, constant
and mixed, in all eight views, on sub-batches between sentinels, on later trips of the grid-stride loop, and through
self-play.  tests/test_area_host.py holds what this file relies on."""
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
import plane_cases as pc

B = pc.B
SENTINEL = 0xA5
B_TRIPS = 533
TRIP_SIZES = (9, 13, 19)


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
    return (('bytes', st, gogame.batch_area_planes), ('tracked', gogame.batch_track(st), gogame.batch_area_planes_tracked))


def check_set(N, c, tag, orient=None):
    """Every `side` form of one set, byte planes and tracked, plain or in the views `orient` (want = the turned expectation)."""
    import torch
    from gymgo_amd import gogame
    n = len(c.states)
    st = mc.to_dev(c.states.copy())         # (the cached arrays are read-only)
    turn = (lambda p: p) if orient is None else (lambda p: pc.turned(p, orient))
    kw = {} if orient is None else {'orient': torch.from_numpy(orient).cuda()}
    side = ae.mixed_side(n)
    want_mixed = np.where(side[:, None, None, None] != 0, c.white, c.black)
    counts_mixed = np.where(side[:, None] != 0, c.counts_white, c.counts_black)
    for name, x, fn in forms(gogame, st):
        for what, s, planes, counts in (('own turn', None, c.planes, c.counts), ('black', np.zeros(n, np.uint8), c.black, c.counts_black),
                                        ('white', np.ones(n, np.uint8), c.white, c.counts_white), ('mixed', side, want_mixed, counts_mixed)):
            got, cnt = fn(x, side=None if s is None else torch.from_numpy(s).cuda(), counts=True, **kw)
            same(got, turn(planes), tag + (name, what))
            same(cnt, counts, tag + (name, what, 'counts'))          # the counts do not turn
            same(fn(x, side=s, **kw), turn(planes), tag + (name, what, 'without counts, side as an array'))
        got, cnt = fn(x, dtype=dtype_of(N), side=side.astype(bool), counts=True, **kw)
        assert got.dtype == dtype_of(N)
        same(got.to(torch.uint8), turn(want_mixed), tag + (name, 'dtype'))
        same(cnt, counts_mixed, tag + (name, 'dtype, counts'))
    black, white = gogame.batch_areas(st)
    same(torch.stack([black, white], dim=1), c.counts_black, tag + ('gogame.batch_areas',))
    if orient is not None:                   # ... and the plain call on the turned boards
        turned = gogame.batch_symmetry(st, kw['orient'] & 7)
        same(turned, pc.turned(c.states, orient), tag + ('batch_symmetry',))
        for name, x, fn in forms(gogame, turned):
            got, cnt = fn(x, counts=True)
            same(got, turn(c.planes), tag + (name, 'the turned position'))
            same(cnt, c.counts, tag + (name, 'the turned position, counts'))


@pytest.mark.gpu
@pytest.mark.parametrize('N', pc.SIZES)
def test_plain_calls_byte_planes_and_tracked(N):
    for kind in pc.SETS:
        check_set(N, ae.case(N, kind), (N, kind))


@pytest.mark.gpu
@pytest.mark.parametrize('N', pc.SIZES)
def test_oriented_calls_byte_planes_and_tracked(N):
    orient = mixed(B)                        # all eight views, with the negative and the large words
    assert set(orient & 7) == set(range(8)) and orient.min() < 0 and orient.max() > 7
    for kind in pc.SETS:
        check_set(N, ae.case(N, kind), (N, kind, 'oriented'), orient)


@pytest.mark.gpu
@pytest.mark.parametrize('N', pc.SIZES)
def test_corridor_boards_plain_and_oriented(N):
    c = ae.case(N, 'corridor')
    cb = ae.corridor_boards(N)
    if N >= 5:
        assert len(c.states) == 32 and cb.plain.sum() == 16
    if not len(c.states):
        return
    check_set(N, c, (N, 'corridor'))
    check_set(N, c, (N, 'corridor', 'oriented'), mixed(len(c.states)))
    # what the boards are there for, read off the device's answer
    from gymgo_amd import gogame
    got = mc.to_np(gogame.batch_area_planes(mc.to_dev(c.states.copy()), side=np.zeros(len(c.states), np.uint8)))
    for i in range(len(c.states)):
        region = cb.corridor[i]
        assert (got[i, int(cb.ring[i]) if cb.plain[i] else 2][region] == 1).all(), (N, i)


@pytest.mark.gpu
@pytest.mark.parametrize('N', pc.SIZES)
def test_sub_batches_between_sentinels(N):
    """A lone board and a wave that is not full, from three places of the batch, written through out= into a slice of a
    larger buffer at 1, 7 or 20 elements into it (out needs its element's alignment only), the counts into a slice of a larger
    int32 buffer.  Nothing before or behind either slice is written.  All four dtypes at every N."""
    import torch
    from gymgo_amd import gogame
    P = N * N

    def room(lead, n, dt):
        size = torch.empty(0, dtype=dt).element_size()
        raw = torch.full(((lead + n) * size + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
        return raw[lead * size:(lead + n) * size].view(dt), lambda: bool((raw[:lead * size] == SENTINEL).all()) and bool(
            (raw[(lead + n) * size:] == SENTINEL).all())

    for j, kind in enumerate(pc.SETS):
        c = ae.case(N, kind)
        st = mc.to_dev(c.states.copy())
        tracked = gogame.batch_track(st)
        side = ae.mixed_side(B)
        want = np.where(side[:, None, None, None] != 0, c.white, c.black)
        want_counts = np.where(side[:, None] != 0, c.counts_white, c.counts_black)
        for nb in (1, 3):
            for k, first in enumerate((0, 7, B - nb)):
                lead, sl = (1, 7, 20)[k], slice(first, first + nb)
                for d, dt in enumerate((torch.uint8, torch.float16, torch.bfloat16, torch.float32)):
                    tag = (N, kind, dt, nb, first)
                    flat, untouched = room(lead, nb * 3 * P, dt)
                    cflat, cuntouched = room(1 + 2 * k, nb * 2, torch.int32)
                    out, cnt = flat.view(nb, 3, N, N), cflat.view(nb, 2)
                    fn, x = ((gogame.batch_area_planes, st), (gogame.batch_area_planes_tracked, tracked))[(k + d + j) % 2]
                    got, gc = fn(x[sl], dtype=dt, out=out, side=side[sl], counts=cnt)
                    assert got is out and gc is cnt
                    same(out.to(torch.uint8), want[sl], tag)
                    same(cnt, want_counts[sl], tag + ('counts',))
                    assert untouched() and cuntouched(), tag


# ---------------------------------------------------------------- later trips of the grid-stride loop
def pool_data(N):
    """The pool of 63 boards - policy ++ clean ++ random - with its expectation from both sides, a mixed `side` vector and
    the views mixed(21)[i mod 21] of pool board i."""
    kinds = ('policy', 'clean', 'random')
    cat = lambda f: np.concatenate([getattr(ae.case(N, k), f) for k in kinds])
    d = {f: cat(f) for f in ('states', 'planes', 'black', 'white', 'counts', 'counts_black', 'counts_white')}
    d['orient'] = np.tile(mixed(B), 3)
    d['side'] = ae.mixed_side(63)
    assert len(d['states']) == 63
    return d


def _trips_child(N, path):
    import torch
    from gymgo_amd import gogame, _lib
    assert _lib.lib().gg_device_cus() == 1
    d = dict(np.load(path))
    i63 = (5 * np.arange(B_TRIPS)) % 63
    st = torch.from_numpy(d['states'][i63]).cuda()
    orient, side = d['orient'][i63], d['side'][i63]
    mix = lambda a, b: np.where(side.reshape((-1,) + (1,) * (d[a].ndim - 1)) != 0, d[a][i63], d[b][i63])
    cases = (('own turn', None, d['planes'][i63], d['counts'][i63]), ('mixed', side, mix('white', 'black'), mix('counts_white', 'counts_black')))

    def room(lead, n, dt):
        size = torch.empty(0, dtype=dt).element_size()
        raw = torch.full(((lead + n) * size + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
        return raw[lead * size:(lead + n) * size].view(dt), lambda: bool((raw[:lead * size] == SENTINEL).all()) and bool(
            (raw[(lead + n) * size:] == SENTINEL).all())

    for form, x, fn in (('bytes', st, gogame.batch_area_planes), ('tracked', gogame.batch_track(st), gogame.batch_area_planes_tracked)):
        for v, o in enumerate((None, orient)):
            for w, (what, s, planes, counts) in enumerate(cases):
                tag = (N, form, 'plain' if o is None else 'oriented', what)
                want = planes if o is None else pc.turned(planes, o)
                flat, untouched = room(1 + 2 * v + 4 * w, want.size, torch.uint8)
                cflat, cuntouched = room(3 + v, counts.size, torch.int32)
                out, cnt = flat.view(want.shape), cflat.view(counts.shape)
                got, gc = fn(x, out=out, orient=o, side=s, counts=cnt)
                assert got is out and gc is cnt, tag
                same(out, want, tag)
                same(cnt, counts, tag + ('counts',))
                assert untouched() and cuntouched(), tag
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


# ---------------------------------------------------------------- ownership and margin
@pytest.mark.gpu
@pytest.mark.parametrize('N', pc.SIZES)
def test_batch_ownership(N):
    import torch
    from gymgo_amd import gogame
    orient = mixed(B)
    side = ae.mixed_side(B)
    for kind in pc.SETS:
        c = ae.case(N, kind)
        st = mc.to_dev(c.states.copy())
        for what, s, planes in (('own turn', None, c.planes), ('black', np.zeros(B, np.uint8), c.black),
                                ('mixed', side, np.where(side[:, None, None, None] != 0, c.white, c.black))):
            own, margin = ae.owner(planes)
            got = gogame.batch_ownership(st, side=s)
            assert isinstance(got, tuple) and len(got) == 2 and got[0].dtype == torch.int8 and got[1].dtype == torch.int32
            same(got[0], own, (N, kind, what, 'owner'))
            same(got[1], margin, (N, kind, what, 'margin'))
            got = gogame.batch_ownership(st, side=s, orient=orient)
            same(got[0], pc.turned(own[:, None], orient)[:, 0], (N, kind, what, 'owner, oriented'))
            same(got[1], margin, (N, kind, what, 'margin does not turn'))
        # NumPy in gives NumPy out; the single-state forms
        own, margin = ae.owner(c.planes)
        got = gogame.batch_ownership(c.states.copy())
        assert isinstance(got[0], np.ndarray) and isinstance(got[1], np.ndarray)
        same(got[0], own, (N, kind, 'numpy')), same(got[1], margin, (N, kind, 'numpy'))
        got = gogame.batch_area_planes(c.states.copy(), counts=True)
        assert isinstance(got[0], np.ndarray) and isinstance(got[1], np.ndarray)
        same(got[0], c.planes, (N, kind, 'numpy planes')), same(got[1], c.counts, (N, kind, 'numpy counts'))
        o1, m1 = gogame.ownership(st[3], side=1)
        w = ae.owner(c.white[3])
        same(o1, w[0], (N, kind, 'single')), same(m1, w[1], (N, kind, 'single margin'))
        p1, c1 = gogame.area_planes(st[4], side=0, counts=True)
        same(p1, c.black[4], (N, kind, 'single planes')), same(c1, c.counts_black[4], (N, kind, 'single counts'))
        same(gogame.area_planes(st[5], dtype=torch.float32).to(torch.uint8), c.planes[5], (N, kind, 'single planes, float32'))


def test_constants_and_value_errors(native_built):
    """Everything here comes before a device is touched."""
    import torch
    from gymgo_amd import gogame, _lib
    assert gogame.AREA_PLANES == 3 == _lib.lib().gg_area_planes() and gogame.AREA_NAMES == ae.NAMES
    L = _lib.lib()
    for fn in (L.gg_batch_area, L.gg_batch_area_tracked):
        assert fn(None, None, None, None, None, 3, 2, 1, None) == -1 and fn(None, None, None, None, None, 4, 2, 9, None) == -1
        assert fn(None, None, None, None, None, 3, 0, 9, None) == 0 and fn(None, None, None, None, None, 3, 2, 9, None) == -2
    st = np.zeros((2, 6, 5, 5), np.uint8)
    for bad in (dict(dtype=torch.float64), dict(orient=[0]), dict(side=[0]), dict(side=[0.0, 1.0]),
                dict(counts=torch.zeros((2, 2), dtype=torch.int32))):
        with pytest.raises(ValueError):
            gogame.batch_area_planes(st, **bad)
    with pytest.raises(ValueError):
        gogame.batch_area_planes(st[:, :5])
    with pytest.raises(ValueError):
        gogame.batch_area_planes(st, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        gogame.batch_ownership(st, side=[1])
    with pytest.raises(ValueError):
        gogame.batch_ownership(st, orient=[1, 2, 3])
    E = lambda planes, legal, *more: None
    dev = torch.zeros((2, 6, 5, 5), dtype=torch.uint8)
    for call in (lambda: gogame.PuctSearch(dev, 3, area=True), lambda: gogame.batch_puct(dev, 3, E, area=True),
                 lambda: gogame.puct_play(dev, 1, 3, E, area=True), lambda: gogame.puct_selfplay(dev, 1, 3, E, area=True),
                 lambda: gogame.puct(dev[0], 3, E, area=True), lambda: gogame.puct_actions(dev, 3, E, area=True)):
        with pytest.raises(ValueError, match='area=True'):
            call()


# ---------------------------------------------------------------- the search
def running_roots(N):
    """The first seven policy positions that have not ended."""
    c = pc.case(N, 'policy')
    idx = np.flatnonzero(c.states[:, 5, 0, 0] == 0)[:7]
    assert len(idx) == 7
    return c.states[idx]


@pytest.mark.gpu
@pytest.mark.parametrize('N', (5, 11))
@pytest.mark.parametrize('more', (False, True))
def test_search_hands_out_the_area_planes_of_its_leaves(N, more):
    import torch
    from gymgo_amd import gogame
    import test_gpu_symmetry_io as tsio
    roots = mc.to_dev(running_roots(N))
    rounds, leaves = 3, 3
    E = tsio.on_device(tsio.point_evaluator)
    kw = dict(life=True, ladder=True, outcome=True) if more else {}
    sa = gogame.PuctSearch(roots, rounds, komi=0.5, leaves=leaves, features=torch.float16, symmetry=99 + N, area=True, **kw)
    sb = gogame.PuctSearch(roots, rounds, komi=0.5, leaves=leaves)          # the states of the same leaves
    seen = np.zeros(3, bool)
    for t in range(rounds):
        res = sa.select()
        assert len(res) == (6 if more else 3)
        planes, legal, area = res[0], res[1], res[-1]
        states, _ = sb.select()
        assert area.dtype == torch.float16 and tuple(area.shape) == (7 * leaves, 3, N, N)
        s, o = mc.to_np(states), mc.to_np(sa.orient)
        assert len(set(o & 7)) > 1
        want = pc.turned(ae.batch_area_planes(s), o)
        same(area.to(torch.uint8), want, (N, t, 'area'))
        seen |= want.any(axis=(0, 2, 3))
        if more:     # the area planes come after life, ladder and outcome
            assert tuple(res[2].shape) == tuple(res[3].shape) == (7 * leaves, 4, N, N) and tuple(res[4].shape) == (7 * leaves, 12, N, N)
            assert bool((res[2].to(torch.uint8) == gogame.batch_life(states, orient=sa.orient)).all()), t
            assert bool((res[3].to(torch.uint8) == gogame.batch_ladder(states, orient=sa.orient)).all()), t
            assert bool((res[4].to(torch.uint8) == gogame.batch_move_planes(states, orient=sa.orient)).all()), t
        priors, values = E(planes, legal)
        sa.backup(priors, values)
        sb.backup(gogame.batch_symmetry_policy(priors, sa.orient, inverse=True), values)
    assert seen[:2].all()
    with pytest.raises(ValueError, match='area=True'):
        gogame.PuctSearch(roots, rounds, area=True)


# ---------------------------------------------------------------- self-play: the area planes and the two targets
SELFPLAY = dict(N=5, R=6, moves=40, iterations=4, komi=0.5, seed=7)


@pytest.mark.gpu
def test_selfplay_batch_with_area_and_ownership():
    import torch
    from gymgo_amd import gogame
    import test_gpu_symmetry_io as tsio
    N, R, M, T, komi = (SELFPLAY[k] for k in ('N', 'R', 'moves', 'iterations', 'komi'))
    roots = mc.to_dev(tsio.roots7(N)[:R])
    kw = dict(c=0.6, komi=komi, capacity=64, sample_moves=4, seed=SELFPLAY['seed'], features=torch.float16, record_states=True)
    rec = gogame.puct_selfplay(roots, M, T, tsio.on_device(tsio.point_evaluator), **kw)
    outcome, lengths = mc.to_np(rec.outcome), mc.to_np(rec.lengths)
    final, states = mc.to_np(rec.final_states), mc.to_np(rec.states)
    ended = final[:, 5, 0, 0] != 0
    # at least one game ended - and one of them on a move played here (seed 7: game 0 after 30 moves, by the CPU restatement
    # tests/mc_puct_selfplay_expect.py)
    assert (ended & (lengths > 0)).any() and (outcome[ended] != 0).all(), (ended, outcome, lengths)
    # a few hundred (game, move, orient) triples: every recorded position once, and a second time in another view
    games, moves = np.tile(np.repeat(np.arange(R), M), 2), np.tile(np.arange(M), 2 * R)
    orient = mixed(2 * R * M)
    orient[R * M:] += 3
    assert len(games) == 480 and set(orient & 7) == set(range(8))
    plain = gogame.selfplay_batch(rec, games, moves, orient)
    full = gogame.selfplay_batch(rec, games, moves, orient, area=True, ownership=True)
    off = gogame.selfplay_batch(rec, games, moves, orient, area=False, ownership=False)
    assert len(plain) == len(off) == 4 and len(full) == 7
    assert all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(off, plain))
    assert all(torch.equal(x, y) for x, y in zip(full[:4], plain))
    area, owner, margin = full[4], full[5], full[6]
    assert area.dtype == torch.float16 and owner.dtype == torch.int8 and margin.dtype == torch.float32
    st = states[games, moves]
    same(area.to(torch.uint8), pc.turned(ae.batch_area_planes(st), orient), 'area planes of the recorded positions')
    white = st[:, 2, 0, 0] != 0
    want_own, want_margin = ae.owner(ae.batch_area_planes(final[games], side=white))
    same(owner, pc.turned(want_own[:, None], orient)[:, 0], 'owner')
    same(margin, want_margin.astype(np.float32), 'margin')
    # for every sample of a game that ended, the sign of the margin with komi is the value target
    z = mc.to_np(full[2])
    score = mc.to_np(margin) + np.where(white, np.float32(komi), np.float32(-komi))
    done = ended[games]
    assert done.any() and white[done].any() and (~white[done]).any()
    assert np.array_equal(np.sign(score[done]), z[done]) and (z[done] != 0).all()
    assert np.array_equal(z[~done], np.zeros((~done).sum(), np.float32))
    # the other orders and dtypes: area after life, ladder and outcome; ownership after everything
    ten = gogame.selfplay_batch(rec, games, moves, orient, dtype=torch.uint8, life=True, ladder=True, outcome=True, area=True,
                                 ownership=True)
    assert len(ten) == 10 and tuple(ten[6].shape) == (480, 12, N, N) and ten[7].dtype == torch.uint8
    assert torch.equal(ten[7], area.to(torch.uint8)) and torch.equal(ten[8], owner) and torch.equal(ten[9], margin)
    six = gogame.selfplay_batch(rec, games, moves, orient, ownership=True)
    assert len(six) == 6 and torch.equal(six[4], owner) and torch.equal(six[5], margin)
    # the search's own planes during self-play: an evaluator that ignores them plays the same games
    calls = []

    def ignore(planes, legal, area_planes):
        calls.append(tuple(area_planes.shape))
        return tsio.on_device(tsio.point_evaluator)(planes, legal)

    again = gogame.puct_selfplay(roots, 3, T, ignore, area=True, **kw)
    short = gogame.puct_selfplay(roots, 3, T, tsio.on_device(tsio.point_evaluator), **kw)
    assert len(calls) == 3 * T and calls[0] == (R, 3, N, N)
    assert all(torch.equal(getattr(again, k), getattr(short, k)) for k in again._fields)
    # a NumPy record gives NumPy samples
    rec_np = type(rec)(*[mc.to_np(x) for x in rec])
    np_full = gogame.selfplay_batch(rec_np, games[:9], moves[:9], orient[:9], area=True, ownership=True)
    assert all(isinstance(x, np.ndarray) for x in np_full) and len(np_full) == 7
    for x, y in zip(np_full, full):
        assert np.array_equal(x, mc.to_np(y)[:9].astype(x.dtype))


if __name__ == '__main__':
    _trips_child(int(sys.argv[1]), sys.argv[2])
