"""-m gpu: the flood-deep boards of tests/flood_plane_cases.py - board-filling snakes captured, put in atari, joined, refused as
suicide, the corridor a capture leaves, spirals, serpentines and combs, every fourth board a random position - through every PLANE
kernel and through the three playout policies at EVERY board size from 2 to 19, bit for bit against the definitional expect
modules.

The failure this file is about: lat_flood (gg_lat.h), the Jacobi flood of every kernel younger than the step kernels, right on the
blobs random play makes - none deeper than about 22 vertical steps - and wrong on a chain 180 steps deep, or at N = 10 .. 12 and
14 .. 18, where a board's lanes hold idle rows and the bit fields of the two colours are wider than the board.  Every entry point
runs on the boards in both forms (forced: plane 3 all ones but q, to be taken as given; genuine: the oracle's plane 3), from byte
planes and from tracked boards, plain and - where it has an `orient` - in the mixed eight views of test_gpu_life.mixed; the output
dtype rotates with N.  The ladder runs on flood_plane_cases.ladder_subset(N) above 12x12.  tests/test_flood_planes_host.py holds
what this file relies on.

The rollouts run twice: in a child process with the library sized for ONE compute unit (GYMGO_AMD_CUS=1, as
tests/test_gpu_flood_sizes.py does: only then the (200, 9) cell reaches the k_rollout5 family at 9 / 13 / 19) and in this process
at the device's own CU count."""
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
import flood_cases as fc
import flood_plane_cases as fp
import mc_expect as mc
import plane_cases as pc
import status_expect as se

SIZES = list(fp.SIZES)


def dtype_of(N):
    import test_gpu_plane_sizes as tps
    return tps.dtype_of(N)


def same(got, want, N, what, rows=None):
    """got == want, row for row; the report names N, the kind and variant of the first boards that differ and their first
    differing points.  rows: the boards of boards(N) the rows belong to (default: all, in order)."""
    import torch
    b = fp.boards(N)
    if torch.is_tensor(got):
        if got.dtype in (torch.float16, torch.bfloat16, torch.float32):
            assert bool(((got == 0) | (got == 1)).all()), (N, what, 'a value that is neither 0 nor 1')
            got = got.to(torch.uint8)
        got = got.cpu().numpy()
    if got.dtype == np.int64 and want.dtype == np.uint64:
        got = got.view(np.uint64)
    assert got.shape == want.shape and got.dtype == want.dtype, (N, what, got.shape, want.shape, got.dtype, want.dtype)
    n = len(got)
    bad = np.flatnonzero((got != want).reshape(n, -1).any(axis=1))
    if len(bad):
        rows = np.arange(n) if rows is None else np.asarray(rows)
        first = [(int(rows[i]), b.kind[rows[i]], int(b.variant[rows[i]]), np.argwhere(np.atleast_1d(got[i] != want[i]))[:6].tolist())
                 for i in bad[:4]]
        raise AssertionError((N, what, '%d of %d boards differ' % (len(bad), n), first))


def device_forms(N, form, rows=None):
    """(byte planes, tracked boards) of one form on the device - after batch_untrack(batch_track(s)) == s, the fact every
    tracked comparison rests on: the tracked words keep plane 3 as it is given"""
    import torch
    from gymgo_amd import gogame
    s = fp.states_of(N, form)
    st = mc.to_dev(s.copy() if rows is None else s[rows])
    tracked = gogame.batch_track(st)
    assert torch.equal(gogame.batch_untrack(tracked), st), (N, form, 'batch_untrack(batch_track(s)) != s')
    return st, tracked


def views(n):
    """(tag, the keywords of the call, what turns the expectation): plain, and the mixed eight views"""
    import torch
    orient = fp.mixed(n)
    assert n < 8 or (set(orient & 7) == set(range(8)) and orient.min() < 0 and orient.max() > 7)
    return (('plain', {}, lambda p: p), ('oriented', {'orient': torch.from_numpy(orient).cuda()}, lambda p: pc.turned(p, orient)))


@pytest.mark.gpu
@pytest.mark.parametrize('N', SIZES)
def test_features_group_liberties_and_life(N):
    from gymgo_amd import gogame
    dt = dtype_of(N)
    for form in fp.FORMS:
        feat, lf = fp.expectation(N, form, 'features'), fp.expectation(N, form, 'life')
        st, tracked = device_forms(N, form)
        same(gogame.batch_group_liberties(st), feat.libs, N, (form, 'group liberties'))
        for tag, kw, turn in views(len(st)):
            for name, x, features, life in (('bytes', st, gogame.batch_features, gogame.batch_life),
                                            ('tracked', tracked, gogame.batch_features_tracked, gogame.batch_life_tracked)):
                same(features(x, dtype=dt, **kw), turn(feat.planes), N, (form, name, tag, 'features', dt))
                got, flags = life(x, dtype=dt, settled=True, **kw)
                same(got, turn(lf.planes), N, (form, name, tag, 'life', dt))
                same(flags, lf.settled, N, (form, name, tag, 'settled'))


@pytest.mark.gpu
@pytest.mark.parametrize('N', SIZES)
def test_ladder(N):
    """Oriented: turned first, then searched, as plane_cases.oriented_ladder does."""
    import torch
    from gymgo_amd import gogame
    dt = dtype_of(N)
    for form in fp.FORMS:
        e = fp.expectation(N, form, 'ladder')
        st, tracked = device_forms(N, form, e.rows)
        planes, aborted = fp.oriented_ladder(N, form)
        orient = torch.from_numpy(fp.mixed(len(e.rows))).cuda()
        for name, x, fn in (('bytes', st, gogame.batch_ladder), ('tracked', tracked, gogame.batch_ladder_tracked)):
            got, ab = fn(x, dtype=dt, aborted=True)
            same(got, e.planes, N, (form, name, 'ladder', dt), e.rows)
            same(ab, e.aborted, N, (form, name, 'aborted'), e.rows)
            got, ab = fn(x, dtype=dt, orient=orient, aborted=True)
            same(got, planes, N, (form, name, 'oriented', 'ladder', dt), e.rows)
            same(ab, aborted, N, (form, name, 'oriented', 'aborted'), e.rows)


@pytest.mark.gpu
@pytest.mark.parametrize('N', SIZES)
def test_move_outcomes_and_hashes(N):
    from gymgo_amd import gogame
    dt = dtype_of(N)
    for form in fp.FORMS:
        out, h = fp.expectation(N, form, 'outcome'), fp.expectation(N, form, 'hash')
        st, tracked = device_forms(N, form)
        same(gogame.batch_move_counts(st), out.counts, N, (form, 'move counts'))
        for name, x, planes, base, moves in (
                ('bytes', st, gogame.batch_move_planes, gogame.batch_hash, gogame.batch_move_hashes),
                ('tracked', tracked, gogame.batch_move_planes_tracked, gogame.batch_hash_tracked, gogame.batch_move_hashes_tracked)):
            for tag, kw, turn in views(len(st)):
                same(planes(x, dtype=dt, **kw), turn(out.planes), N, (form, name, tag, 'move planes', dt))
            same(base(x), h.hashes, N, (form, name, 'hash'))
            same(moves(x), h.moves, N, (form, name, 'move hashes'))


def sides(n, c):
    """(tag, side, planes, counts) of an expectation with .planes / .black / .white and their counts: absent, constant, mixed"""
    side = ae.mixed_side(n)
    return (('own turn', None, c.planes, c.counts), ('black', np.zeros(n, np.uint8), c.black, c.counts_black),
            ('white', np.ones(n, np.uint8), c.white, c.counts_white),
            ('mixed', side, np.where(side[:, None, None, None] != 0, c.white, c.black), np.where(side[:, None] != 0, c.counts_white, c.counts_black)))


@pytest.mark.gpu
@pytest.mark.parametrize('N', SIZES)
def test_area_and_stone_status(N):
    import torch
    from gymgo_amd import gogame
    dt = dtype_of(N)
    for form in fp.FORMS:
        area, status = fp.expectation(N, form, 'area'), fp.expectation(N, form, 'status')
        st, tracked = device_forms(N, form)
        n = len(st)
        for tag, kw, turn in views(n):
            for name, x, fa, fs in (('bytes', st, gogame.batch_area_planes, gogame.batch_stone_status),
                                    ('tracked', tracked, gogame.batch_area_planes_tracked, gogame.batch_stone_status_tracked)):
                for what, s, planes, counts in sides(n, area):
                    s = None if s is None else torch.from_numpy(s).cuda()
                    got, cnt = fa(x, dtype=dt, side=s, counts=True, **kw)
                    same(got, turn(planes), N, (form, name, tag, what, 'area', dt))
                    same(cnt, counts, N, (form, name, tag, what, 'area counts'))           # the counts do not turn
                for thr in se.THRESHOLDS:
                    c = status.by[thr]
                    own = mc.to_dev(c.own.copy())         # in the stored frame, whatever the view
                    for what, s, planes, counts in sides(n, c):
                        s = None if s is None else torch.from_numpy(s).cuda()
                        got, cnt = fs(x, own, c.K, thr, dtype=dt, side=s, counts=True, **kw)
                        same(got, turn(planes), N, (form, name, tag, what, thr, 'status', dt))
                        same(cnt, counts, N, (form, name, tag, what, thr, 'status counts'))


@pytest.mark.gpu
@pytest.mark.parametrize('N', SIZES)
def test_tactics_patterns_priors_and_eyes(N):
    from gymgo_amd import gogame
    dt = dtype_of(N)
    for form in fp.FORMS:
        tac, pat, pri = (fp.expectation(N, form, f) for f in ('tactics', 'patterns', 'priors'))
        st, tracked = device_forms(N, form)
        n = len(st)
        same(gogame.batch_eye_mask(st), fp.expectation(N, form, 'eyes').mask, N, (form, 'eye mask'))
        for name, x, tactics, patterns, priors in (
                ('bytes', st, gogame.batch_tactics, gogame.batch_patterns, gogame.batch_move_priors),
                ('tracked', tracked, gogame.batch_tactics_tracked, gogame.batch_patterns_tracked, gogame.batch_move_priors_tracked)):
            for ln, last in fp.last_variants(N, n):
                for tag, kw, turn in views(n):
                    if ln == 'none':
                        same(tactics(x, dtype=dt, **kw), turn(tac.planes), N, (form, name, tag, 'tactics', dt))
                    same(patterns(x, last, dtype=dt, **kw), turn(pat.by[ln]), N, (form, name, tag, 'patterns', ln, dt))
                for wn, w in fp.PRIORS:
                    same(priors(x, gogame.UctPrior(*w), last=last), pri.by[wn, ln], N, (form, name, 'priors', wn, ln))


# ---------------------------------------------------------------- the playout policies: rollouts
def rollout_cells():
    return [(policy, B, plies, auto) for policy in fp.POLICIES for B, plies in fp.ROLLOUT_CELLS for auto in (True, False)]


def _key(policy, B, plies, auto):
    return '%s_%d_%d_%d' % (policy, B, plies, auto)


def expected_rollouts(N):
    """name -> array, for np.savez: boards, generators and last actions of every cell by the CPU rollouts of the policy modules"""
    out = {}
    for cell in rollout_cells():
        for part, a in zip(('states', 'rng', 'last'), fp.rollout(N, *cell)):
            out[_key(*cell) + '_' + part] = a
    return out


def run_rollouts(N, want):
    """batch_rollout_tracked of every cell from the first B boards of flood_cases.batch(N): the untracked boards, the tracked
    words (those of batch_track of the expected boards: the liberty classes are a function of the position), the generators and
    the last actions"""
    import torch
    from gymgo_amd import gogame
    b = fc.batch(N)
    dev = torch.from_numpy(b.states).cuda()

    def equal(got, want, *what):
        got = got.cpu().numpy()
        if want.dtype == np.uint64:
            got = got.view(np.uint64)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
        first = [(int(i), b.kind[i], int(fc.cases(N).variant[b.index[i]]) if b.index[i] >= 0 else -1,
                  np.argwhere(np.atleast_1d(got[i] != want[i]))[:6].tolist()) for i in bad[:4]]
        assert len(bad) == 0, (N,) + what + ('%d of %d boards differ' % (len(bad), len(got)), first)

    for policy, B, plies, auto in rollout_cells():
        k = _key(policy, B, plies, auto)
        tr, rng = gogame.batch_track(dev[:B]), gogame.rng_seed(B, fc.SEED, 0, 'cuda')
        equal(rng, fp.generators(B), 'generators before', k)
        la = torch.from_numpy(fp.last_before(policy, N, B)).cuda()
        gogame.batch_rollout_tracked(tr, rng, plies, auto, la, policy=policy)
        equal(gogame.batch_untrack(tr), want[k + '_states'], 'boards', k)
        equal(tr, gogame.batch_track(mc.to_dev(want[k + '_states'].copy())).cpu().numpy(), 'tracked words', k)
        equal(rng, want[k + '_rng'], 'generators', k)
        equal(la, want[k + '_last'], 'last actions', k)
    torch.cuda.synchronize()


def _rollout_child(N, path):
    from gymgo_amd import _lib
    assert _lib.lib().gg_device_cus() == 1
    run_rollouts(N, dict(np.load(path)))
    print('FLOOD ROLLOUTS ' + json.dumps({'N': N, 'ok': True}))


@pytest.mark.gpu
@pytest.mark.parametrize('N', SIZES)
def test_policy_rollouts_on_one_compute_unit_and_on_the_whole_device(N, tmp_path):
    want = expected_rollouts(N)
    path = str(tmp_path / 'rollouts.npz')
    np.savez(path, **want)
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '1'
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(N), path], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith('FLOOD ROLLOUTS ')][-1]
    assert json.loads(line[len('FLOOD ROLLOUTS '):]) == {'N': N, 'ok': True}
    run_rollouts(N, want)


# ---------------------------------------------------------------- the playout policies: playouts
@pytest.mark.gpu
@pytest.mark.parametrize('N', SIZES)
def test_playouts_from_one_root_of_each_kind_and_colour(N):
    from gymgo_amd import gogame
    b = fp.boards(N)
    rows, roots = fp.playout_roots(N)
    dev = mc.to_dev(roots.copy())
    named = [(int(i), b.kind[i], int(b.variant[i])) for i in rows]
    for policy in ('uniform',) + fp.POLICIES:
        want = fp.playouts(N, policy)
        for slots in fp.PLAYOUT_SLOTS:
            got = gogame.batch_playouts(dev, fp.PLAYOUTS, max_plies=fp.PLAYOUT_PLIES, ownership=True, slots=slots,
                                        chunk_plies=fp.PLAYOUT_PLIES, policy=policy)
            mc.check(got, want, mc.KEYS + ('ownership',), (N, policy, slots, 'roots', named))
    assert bool((dev == mc.to_dev(roots.copy())).all())


if __name__ == '__main__':
    _rollout_child(int(sys.argv[1]), sys.argv[2])
