"""-m gpu: the plane kernels PAST ONE GRID.  plane_launch (gg_planes.h) starts at most 64 single-wave workgroups per compute
unit, each of four boards (N <= 13) or two; the rest of the batch goes through the grid-stride loop of k_features*,
k_group_liberties, k_life, k_ladder, k_moves, k_hash and k_move_hashes - on a 256-CU device only above 65 536 / 32 768 boards,
and the other plane tests use a few dozen.  What a second trip of that loop can get wrong: the LDS staging buffer, the
bit-string, the ladder's take-back stack and the lcand / lrep words of k_move_hashes reused after an earlier trip; a ragged last
group on a late trip (PlaneFrame::on, the B - 1 clamp of the tracked loads); an output offset past the first grid.

1. One child process per board size 2 .. 19 with the library sized for ONE compute unit (GYMGO_AMD_CUS=1: a grid of 64
   workgroups) and 533 boards: 134 groups of four - workgroups 0 .. 5 make three trips, the last group holds one board on
   workgroup 5's third trip - or 267 groups of two: up to five trips, the last group one board on workgroup 10's fifth.  Board b
   is board 5 b mod 42 of the policy and clean sets of tests/plane_cases.py (5 b mod 63 with the random set, for features,
   liberties and life), so a wave's boards differ and so do a workgroup's successive trips; the expectation is the same gather
   of the definitional expectations, which the parent hands to the child in a file.  Every call writes between sentinels.
2. At the device's own CU count, N = 9, 13, 19 on cus * 64 * nbw + 3 * nbw + 1 boards from device rollouts of mixed depths: a
   few workgroups make a second trip, the last group is ragged.  The whole batch in one call must equal the same call on
   chunks of 4 096 boards, which stay below the cap.  And one output that crosses 2^31 bytes.
   Measured on an MI355X (256 CUs), one ladder call on the whole batch: 4 ms at 9x9 and 7 ms at 13x13 (65 549 boards), 11 ms at
   19x19 (32 775 boards) - the ladder stays in at all three sizes.
"""
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

SIZES = tuple(range(2, 20))
B_TRIPS = 533
SUB_FIRST, SUB_B = 3, 257
SENTINEL = 0xA5


# ---------------------------------------------------------------- 1. the parent's side: the pools and their expectation
def pool_data(N):
    """The two pools - 42: policy ++ clean, 63: policy ++ clean ++ random - with the cached definitional expectations of their
    boards, the oriented ones in view mixed(21)[i mod 21] of pool board i, and a history per board built by
    test_gpu_hash.mask_case."""
    import hash_expect as he
    import outcome_expect as oe
    import plane_cases as pc
    import test_gpu_hash as tgh
    import test_gpu_life as tgl
    o21 = tgl.mixed(pc.B)
    k42, k63 = ('policy', 'clean'), ('policy', 'clean', 'random')
    cat = lambda kinds, f: np.concatenate([f(k) for k in kinds])
    d = {'orient42': np.tile(o21, 2), 'orient63': np.tile(o21, 3)}
    for name, kinds in (('42', k42), ('63', k63)):
        d['states' + name] = cat(kinds, lambda k: pc.case(N, k).states)
    for f in ('features', 'libs', 'life', 'settled'):
        d[f + '63'] = cat(k63, lambda k: getattr(pc.case(N, k), f))
    for f in ('ladder', 'aborted'):
        d[f + '42'] = cat(k42, lambda k: getattr(pc.case(N, k), f))
    d['counts42'], d['mplanes42'] = cat(k42, lambda k: oe.case(N, k).counts), cat(k42, lambda k: oe.case(N, k).planes)
    d['hashes42'], d['moves42'] = cat(k42, lambda k: he.case(N, k).hashes), cat(k42, lambda k: he.case(N, k).moves)
    d['ofeatures63'], d['olife63'] = pc.turned(d['features63'], d['orient63']), pc.turned(d['life63'], d['orient63'])
    d['omplanes42'] = pc.turned(d['mplanes42'], d['orient42'])
    turned = [pc.oriented_ladder(N, k, tuple(int(v) for v in o21)) for k in k42]
    d['oladder42'], d['oaborted42'] = np.concatenate([t[0] for t in turned]), np.concatenate([t[1] for t in turned])
    masks = [tgh.mask_case(N, k) for k in k42]
    d['history42'], d['count42'] = np.concatenate([m[1] for m in masks]), np.concatenate([m[2] for m in masks])
    d['repeat42'] = np.concatenate([he.batch_repeat(m[0].states, m[0].moves, m[1], m[2]) for m in masks])
    d['rows42'] = he.rows_of(d['repeat42'], N)
    assert d['repeat42'].any() and len(d['states42']) == 42 and len(d['states63']) == 63
    return d


# ---------------------------------------------------------------- 1. the child's side
def _room(n, dt, lead):
    """a buffer of sentinels and the `n` elements of dtype dt that start `lead` elements into it"""
    import torch
    size = torch.empty(0, dtype=dt).element_size()
    raw = torch.full(((lead + n) * size + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
    return raw, raw[lead * size:(lead + n) * size].view(dt), lambda: bool((raw[:lead * size] == SENTINEL).all()) and bool(
        (raw[(lead + n) * size:] == SENTINEL).all())


def _same(got, want, tag):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
    assert len(bad) == 0, (tag, len(bad), 'boards', bad[:12].tolist())


def _trips_child(N, path):
    import torch
    from gymgo_amd import gogame, _lib
    assert _lib.lib().gg_device_cus() == 1
    d = dict(np.load(path))
    P, A = N * N, N * N + 1
    u8, f32, i64, i32 = torch.uint8, torch.float32, torch.int64, torch.int32
    stream = lambda: _lib.stream_ptr(torch.device('cuda', torch.cuda.current_device()))

    def planes(fn, x, want, dt, lead, tag, orient=None, flag=None, want_flag=None):
        raw, flat, untouched = _room(want.size, dt, lead)
        out = flat.view(want.shape)
        kw = {} if orient is None else {'orient': orient}
        if flag:
            res, f = fn(x, dtype=dt, out=out, **kw, **{flag: True})
            _same(f, want_flag, tag + (flag,))
        else:
            res = fn(x, dtype=dt, out=out, **kw)
        assert res is out, tag
        _same(out.to(u8), want, tag)
        assert untouched(), tag

    def raw_call(name, x, want, dt, lead, tag):
        """an entry point whose wrapper has no out=: (boards, out, B, N, stream)"""
        _, flat, untouched = _room(want.size, dt, lead)
        out = flat.view(want.shape)
        _lib.call(name, x, out, len(want), N, stream())
        _same(out, want, tag)
        assert untouched(), tag

    def move_hashes(name, x, idx, tag):
        """hashes, repeat and rows of one launch, each between sentinels"""
        n = len(idx)
        hist = torch.from_numpy(np.ascontiguousarray(d['history42'][idx])).cuda()
        count = torch.from_numpy(np.ascontiguousarray(d['count42'][idx])).cuda()
        rooms = [_room(n * A, i64, 3), _room(n * A, u8, 5), _room(n * N, i32, 7)]
        _lib.call(name, x, hist, count, hist.shape[1], rooms[0][1], rooms[1][1], rooms[2][1], n, N, stream())
        _same(rooms[0][1].view(n, A), d['moves42'][idx], tag + ('hashes',))
        _same(rooms[1][1].view(n, A), d['repeat42'][idx], tag + ('repeat',))
        _same(rooms[2][1].view(n, N), d['rows42'][idx], tag + ('rows',))
        assert all(r[2]() for r in rooms), tag

    b = np.arange(B_TRIPS)
    i42, i63 = (5 * b) % 42, (5 * b) % 63
    st42, st63 = torch.from_numpy(d['states42'][i42]).cuda(), torch.from_numpy(d['states63'][i63]).cuda()
    tr42, tr63 = gogame.batch_track(st42), gogame.batch_track(st63)
    _same(gogame.batch_untrack(tr42), d['states42'][i42], (N, 'track and back'))
    o42, o63 = torch.from_numpy(d['orient42'][i42]).cuda(), torch.from_numpy(d['orient63'][i63]).cuda()
    w = lambda key, idx: d[key][idx]
    for form, x42, x63, sfx in (('bytes', st42, st63, ''), ('tracked', tr42, tr63, '_tracked')):
        g = lambda name: getattr(gogame, name + sfx)
        tag = (N, form)
        planes(g('batch_features'), x63, w('features63', i63), u8, 16, tag + ('features',))
        planes(g('batch_features'), x63, w('features63', i63), f32, 4, tag + ('features, float32',))
        planes(g('batch_features'), x63, w('ofeatures63', i63), u8, 32, tag + ('features, oriented',), orient=o63)
        planes(g('batch_life'), x63, w('life63', i63), u8, 1, tag + ('life',), flag='settled', want_flag=w('settled63', i63))
        planes(g('batch_life'), x63, w('olife63', i63), u8, 7, tag + ('life, oriented',), orient=o63, flag='settled',
               want_flag=w('settled63', i63))
        planes(g('batch_ladder'), x42, w('ladder42', i42), u8, 3, tag + ('ladder',), flag='aborted', want_flag=w('aborted42', i42))
        planes(g('batch_ladder'), x42, w('oladder42', i42), u8, 9, tag + ('ladder, oriented',), orient=o42, flag='aborted',
               want_flag=w('oaborted42', i42))
        planes(g('batch_move_planes'), x42, w('mplanes42', i42), u8, 5, tag + ('move planes',))
        planes(g('batch_move_planes'), x42, w('omplanes42', i42), u8, 11, tag + ('move planes, oriented',), orient=o42)
        raw_call('gg_batch_hash' + sfx, x42, w('hashes42', i42), i64, 3, tag + ('hash',))
        move_hashes('gg_batch_move_hashes' + sfx, x42, i42, tag + ('move hashes',))
        # the sub-batch: the ragged group on another workgroup and trip
        sl = slice(SUB_FIRST, SUB_FIRST + SUB_B)
        planes(g('batch_features'), x63[sl], w('features63', i63[sl]), u8, 16, tag + ('features, sub-batch',))
        move_hashes('gg_batch_move_hashes' + sfx, x42[sl], i42[sl], tag + ('move hashes, sub-batch',))
    raw_call('gg_batch_group_liberties', st63, w('libs63', i63), u8, 13, (N, 'group liberties'))
    raw_call('gg_batch_move_counts', st42, w('counts42', i42), u8, 15, (N, 'move counts'))
    torch.cuda.synchronize()
    print('TRIPS ' + json.dumps({'N': N, 'ok': True}))


def _child(N, path):
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '1'
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(N), path], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith('TRIPS ')][-1]
    return json.loads(line[len('TRIPS '):])


@pytest.mark.gpu
@pytest.mark.parametrize('N', SIZES)
def test_every_plane_kernel_on_later_trips_of_its_loop(N, tmp_path):
    nbw = 4 if N <= 13 else 2
    groups = (B_TRIPS + nbw - 1) // nbw
    assert groups == (134 if nbw == 4 else 267) and B_TRIPS % nbw == 1 and (groups - 1) % 64 == (5 if nbw == 4 else 10)
    path = str(tmp_path / 'pools.npz')
    np.savez(path, **pool_data(N))
    assert _child(N, path) == {'N': N, 'ok': True}


# ---------------------------------------------------------------- 2. at the device's own CU count
CHUNK = 4096
OWN_SIZES = (9, 13, 19)
LADDER_SIZES = (9, 13, 19)


def device_positions(N, B, seed=5):
    """uint8 [B, 6, N, N] on the device: eight parts of the batch after 3, 14, .. 80 plies of uniform play (auto_reset on)"""
    from gymgo_amd import gogame
    st, rng = gogame.batch_init_state(B, N, device='cuda'), gogame.rng_seed(B, seed)
    ch = B // 8
    for g in range(8):
        hi = B if g == 7 else (g + 1) * ch
        gogame.batch_rollout(st[g * ch:hi], rng[g * ch:hi], 11 * g + 3, True)
    return st


def chunked(fn, B):
    """fn(lo, hi) -> a tensor or a tuple of tensors, over chunks of CHUNK boards, concatenated"""
    import torch
    parts = [fn(lo, min(B, lo + CHUNK)) for lo in range(0, B, CHUNK)]
    if isinstance(parts[0], tuple):
        return tuple(torch.cat([p[i] for p in parts]) for i in range(len(parts[0])))
    return torch.cat(parts)


def equal(whole, parts, tag):
    import torch
    if not isinstance(whole, tuple):
        whole, parts = (whole,), (parts,)
    for i, (a, b) in enumerate(zip(whole, parts)):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (tag, i, torch.nonzero((a != b).reshape(len(a), -1).any(dim=1))[:8].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize('N', OWN_SIZES)
def test_a_batch_past_the_grid_equals_its_chunks(N):
    import torch
    from gymgo_amd import gogame, _lib
    cus = int(_lib.lib().gg_device_cus())
    assert cus == torch.cuda.get_device_properties(0).multi_processor_count
    nbw = 4 if N <= 13 else 2
    B = cus * 64 * nbw + 3 * nbw + 1
    assert CHUNK < cus * 64 * nbw
    P, u8 = N * N, torch.uint8
    st = device_positions(N, B)
    tr = gogame.batch_track(st)
    orient = (torch.arange(B, device='cuda', dtype=torch.int32) * 3 + 1) % 8
    assert bool((st[-1, :2] != 0).any())                                          # the lone board of the ragged group holds stones
    for form, x, sfx in (('bytes', st, ''), ('tracked', tr, '_tracked')):
        g = lambda name: getattr(gogame, name + sfx)
        calls = [('features', lambda lo, hi: g('batch_features')(x[lo:hi], dtype=u8)),
                 ('features, oriented', lambda lo, hi: g('batch_features')(x[lo:hi], dtype=u8, orient=orient[lo:hi])),
                 ('life', lambda lo, hi: g('batch_life')(x[lo:hi], settled=True)),
                 ('life, oriented', lambda lo, hi: g('batch_life')(x[lo:hi], orient=orient[lo:hi], settled=True)),
                 ('move planes', lambda lo, hi: g('batch_move_planes')(x[lo:hi])),
                 ('move planes, oriented', lambda lo, hi: g('batch_move_planes')(x[lo:hi], orient=orient[lo:hi])),
                 ('hash', lambda lo, hi: g('batch_hash')(x[lo:hi])),
                 ('move hashes', lambda lo, hi: g('batch_move_hashes')(x[lo:hi]))]
        if N in LADDER_SIZES:
            calls += [('ladder', lambda lo, hi: g('batch_ladder')(x[lo:hi], aborted=True)),
                      ('ladder, oriented', lambda lo, hi: g('batch_ladder')(x[lo:hi], orient=orient[lo:hi], aborted=True))]
        if not sfx:
            calls += [('group liberties', lambda lo, hi: gogame.batch_group_liberties(x[lo:hi])),
                      ('move counts', lambda lo, hi: gogame.batch_move_counts(x[lo:hi]))]
        for name, fn in calls:
            equal(fn(0, B), chunked(fn, B), (N, form, name))
        # the repeat mask and its rows: per board a history of its own hash, the children of two points and a decoy
        moves = chunked(lambda lo, hi: g('batch_move_hashes')(x[lo:hi]), B)
        b = torch.arange(B, device='cuda')
        hist = torch.stack([moves[b, (7 * b) % P], moves[:, P], moves[b, (11 * b + 3) % P], b * 0x9E3779B97F4A7C1 + 1], dim=1).contiguous()
        count = torch.tensor([4, 3, 0, 9, -1], dtype=torch.int32, device='cuda')[b % 5].contiguous()
        both = lambda lo, hi: gogame._move_hashes(x[lo:hi], bool(sfx), (hist[lo:hi], count[lo:hi]), repeat=True, rows=True)[2:]
        whole = both(0, B)
        assert bool(whole[0].any()) and bool(whole[1].any()), (N, form)
        equal(whole, chunked(both, B), (N, form, 'repeat and rows'))


@pytest.mark.gpu
def test_an_output_that_crosses_two_to_the_31_bytes():
    """batch_features in float32 at 19x19 on 93 000 boards: 2.15 GB in one call against the same boards in chunks."""
    import torch
    from gymgo_amd import gogame
    N, B = 19, 93000
    assert B * 16 * N * N * 4 > 2 ** 31 > (B - CHUNK) * 16 * N * N * 4 - 2 ** 28
    st = device_positions(N, B, seed=6)
    whole = gogame.batch_features(st, dtype=torch.float32)
    parts = torch.empty_like(whole)
    for lo in range(0, B, CHUNK):
        hi = min(B, lo + CHUNK)
        gogame.batch_features(st[lo:hi], dtype=torch.float32, out=parts[lo:hi])
    assert bool(whole[-1, 15].all()) and bool((whole[-1, :2] != 0).any())       # the last board, past 2^31 bytes, is written
    assert torch.equal(whole, parts)
    del whole, parts, st
    torch.cuda.empty_cache()


if __name__ == '__main__':
    _trips_child(int(sys.argv[1]), sys.argv[2])
